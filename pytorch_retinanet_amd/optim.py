"""``MasterSGD`` -- ``torch.optim.SGD`` (the reference's optimizer, ``hparams.yaml:63-68``) on fp32 master weights,
with the convolution weights of the model held in bf16 for the autocast forward.

Why: under bf16 autocast PyTorch re-casts every fp32 conv weight to bf16 in each forward and every bf16 weight
gradient back to fp32 in each backward (94 + 92 small kernels per R50-FPN step), then runs the foreach SGD kernels.
``use_bf16_conv_weights(model)`` swaps every 4-D fp32 conv weight for its bf16 rounding (what autocast would have
fed the convolution anyway) and parks the fp32 tensor as the parameter's master; ``MasterSGD.step()`` does the
whole update in fp32 on the masters -- same arithmetic and order as ``torch.optim.SGD`` -- and refreshes the bf16
copies, for all parameters in one HIP launch per 48 tensors (``rn_sgd_master_step``, ``csrc/optim.hip``).
The trajectory is the autocast + SGD one (fp32 masters, bf16-rounded weights in the forward, bf16 weight gradients
promoted exactly); a converted model must run under autocast.  ``master_state_dict`` / ``load_master_state_dict``
give and take fp32 checkpoints with the reference's keys.

``MasterAdam`` / ``MasterAdamW`` do the same for ``torch.optim.Adam`` / ``AdamW`` (``rn_adam_master_step``, ``csrc/adam.hip``), with every
hyperparameter and the step counter in a device block per parameter group: a captured step follows a per-step LR schedule.
``MasterSGD(capturable=True)`` does the same for SGD (``rn_sgd_master_step_dev``): the bits of the by-value step, read from a block.

``GradClip`` -- ``torch.nn.utils.clip_grad_norm_`` for the three of them (``rn_grad_norm_clip``, ``csrc/clip.hip``): one read of every
gradient gives the global L2 norm and the clip coefficient in a device block, and the step kernels multiply the coefficient into each
gradient as they read it.  No gradient is rewritten, nothing synchronises, and ``max_norm`` lives on the device: the clipped step
captures like the plain one.

``GradAccumulator`` -- Lightning's ``accumulate_grad_batches`` for the three of them (``rn_grad_accumulate``, ``csrc/accum.hip``): the
gradients of N micro-batches summed into fp32 accumulators (never in 16 bits), the window position, 1 / N and found_inf in a device
block, the optimizer stepping on the accumulators through ``step(grads=...)``: one micro graph and one final graph per batch signature.

``WeightEMA`` -- an exponential moving average of the fp32 weights for the three of them (``rn_ema_update``, ``csrc/ema.hip``; torchvision's
``--model-ema``, timm's ``ModelEma``): installed as ``optimizer.weight_ema`` it is updated inside ``step()`` -- skipped with the step under a
loss scaler, part of a captured step -- with the decay schedule and the update count in a device block; ``swapped()`` exchanges it with the
training weights for evaluation and checkpoints.
"""
import contextlib
import ctypes as C
from typing import Dict, Iterable, List, Optional

import numpy as np
import torch
from torch import Tensor, nn

from ._lib import RN_BF16, RN_F16, check, lib
from .norm import note_raw_write


def use_16bit_conv_weights(model: nn.Module, dtype: torch.dtype = torch.bfloat16) -> int:
    """Convert every 4-D fp32 parameter (conv weights) to ``dtype`` (bf16 or fp16: the autocast dtype of the run) in place, keeping the
    fp32 values as ``p.master``.  Returns the number of converted parameters.  BatchNorm parameters and biases stay fp32."""
    if dtype not in (torch.bfloat16, torch.float16):
        raise TypeError(f"working copies are bf16 or fp16, not {dtype}")
    n = 0
    for p in model.parameters():
        if p.dim() == 4 and p.dtype == torch.float32 and p.is_cuda:
            master = p.data
            p.data = master.to(dtype)                     # preserves the memory format (channels_last stays)
            p.master = master
            if p.grad is not None:
                p.grad = None
            n += 1
    return n


def use_bf16_conv_weights(model: nn.Module) -> int:
    return use_16bit_conv_weights(model, torch.bfloat16)


def master_state_dict(model: nn.Module) -> Dict[str, Tensor]:
    "``model.state_dict()`` with every converted weight replaced by its fp32 master (checkpoint format of the reference)."
    sd = model.state_dict()
    for name, p in model.named_parameters():
        if hasattr(p, "master"):
            sd[name] = p.master.detach().clone()
    return sd


def load_master_state_dict(model: nn.Module, state: Dict[str, Tensor], strict: bool = True):
    "Load an fp32 checkpoint into a converted model: masters take the fp32 values, the bf16 copies their rounding."
    out = model.load_state_dict({k: v for k, v in state.items()}, strict=strict)      # copies (rounding) into the bf16 params
    with torch.no_grad():
        for name, p in model.named_parameters():
            if hasattr(p, "master") and name in state:
                p.master.copy_(state[name])
                p.data.copy_(p.master)
    return out


def _is_capturing() -> bool:
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


def _device_block(blk: Optional[Tensor], n: int, device: torch.device, in_capture: str, elsewhere: str) -> Tensor:
    """``blk``, or -- the first time -- a zeroed ``float64[n]`` on ``device`` for its owner to keep for good (captured steps hold its
    address: it is never moved or replaced).  Not created inside a capture (``in_capture``: the owner's message) and not used from a
    second device (``elsewhere``, formatted with ``have`` / ``want``)."""
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if blk is None:
        if _is_capturing():
            raise RuntimeError(in_capture)
        return torch.empty(n, dtype=torch.float64, device=device).fill_(0)      # (a fill kernel, not a memset: graph.py)
    if blk.device != device:
        raise RuntimeError(elsewhere.format(have=blk.device, want=device))
    return blk


def _collect(params: Iterable[Tensor], grads: Optional[Dict[Tensor, Tensor]], refuse, state, **rec) -> Optional[dict]:
    """One walk over ``params`` for a multi-tensor launch: the gradient of each (``grads[p]`` wins over ``p.grad``), its fp32 tensor
    (``p.master`` behind a 16-bit working copy, else ``p.data``), the dtype checks, and the gradient brought to that tensor's strides.
    Returns ``rec`` with ``masters`` / ``gptrs`` / ``p16s`` / ``ns``, ``grads16`` (the gradients of the 16-bit parameters are 16-bit too), ``dt16``,
    ``dev`` and ``keep`` (the re-laid-out gradients: they must outlive the launch) -- or None when no parameter has a gradient.
    ``refuse(cpu)``: the user's exception for a CPU tensor (True) or a tensor that is not fp32 (False).  ``state(rec, p, w)``: the
    user's hook, called after those checks to create its per-parameter state and add its own pointers to ``rec``; ``w`` is None for
    a parameter without a gradient."""
    rec.update(masters=[], gptrs=[], p16s=[], ns=[], grads16=None, dt16=None, keep=[], dev=None)
    for p in params:
        g = grads.get(p) if grads is not None else None
        if g is None:
            g = p.grad
        if g is None:
            state(rec, p, None)
            continue
        has16 = hasattr(p, "master")
        w = p.master if has16 else p.data
        if not (p.is_cuda and g.is_cuda):
            raise refuse(True)
        if w.dtype != torch.float32:
            raise refuse(False)
        state(rec, p, w)
        if has16:
            if rec["dt16"] is None:
                rec["dt16"] = p.dtype
            elif rec["dt16"] != p.dtype:
                raise RuntimeError("the 16-bit working copies of one launch must share a dtype")
            is16 = g.dtype == p.dtype
            if not is16 and g.dtype != torch.float32:
                raise TypeError(f"unsupported gradient dtype {g.dtype} for a {p.dtype} working copy")
            if rec["grads16"] is None:
                rec["grads16"] = is16
            elif rec["grads16"] != is16:
                raise RuntimeError("gradients of the 16-bit parameters must be all 16-bit or all fp32")
        elif g.dtype != torch.float32:
            raise TypeError("fp32 parameters need fp32 gradients")
        # same memory order for the fp32 tensor, the optimizer's state, the gradient and the 16-bit copy: all carry the parameter's strides
        if g.stride() != w.stride():
            g = g.contiguous(memory_format=torch.channels_last) if w.dim() == 4 and w.is_contiguous(memory_format=torch.channels_last) \
                else g.contiguous()
            rec["keep"].append(g)
        if rec["dev"] is None:
            rec["dev"] = w.device
        rec["masters"].append(w.data_ptr()); rec["gptrs"].append(g.data_ptr()); rec["p16s"].append(p.data.data_ptr() if has16 else 0); rec["ns"].append(w.numel())
    return rec if rec["ns"] else None


def _ptrs(values: List[int]):
    return (C.c_void_p * len(values))(*values)


def _dt16(dtype) -> int:
    return RN_F16 if dtype == torch.float16 else RN_BF16


RN_CLIP_STATE = 8                       # doubles in the clip block (include/retinanet_hip.h)
RN_CLIP_CHUNK = 16384                   # elements per scratch slot
_CLIP_COEF_BYTE = 8                     # byte offset of clip_coef in the block


class GradClip:
    """Gradient clipping by global L2 norm for ``MasterSGD`` / ``MasterAdam`` / ``MasterAdamW`` -- what ``torch.nn.utils.clip_grad_norm_``
    (Lightning's ``gradient_clip_val``) does between backward and the optimizer step, without rewriting a gradient.  Install it as
    ``optimizer.grad_clip`` (or construct the optimizer with ``max_grad_norm=``); every ``step()`` then makes one ``rn_grad_norm_clip``
    call over the gradients of all parameter groups and the step kernels scale each gradient by the coefficient they read from this
    object's device block: ``g = (float(grad) / grad_scale) * clip_coef``, in fp32, before weight decay.

    The block and the scratch buffer of partial sums are created at the first step, on the device of the first gradient -- not
    inside a capture -- and kept for good (a captured step holds their addresses).  ``max_norm`` lives in the block: assigning it
    is one tiny launch and the next replay of a captured step clips at the new value.  ``total_norm`` / ``clip_coef`` are views into
    the block (reading them synchronises, like any device tensor); ``stats()`` reads the three counters.  Under a ``GradScaler``
    the norm is of the UNSCALED gradients; nobody calls ``unscale_``."""

    def __init__(self, max_norm: float, norm_type: float = 2.0):
        if float(norm_type) != 2.0:
            raise ValueError(f"GradClip clips by the global L2 norm only (norm_type=2.0), got norm_type={norm_type}")
        self._max_norm = self._check_max_norm(max_norm)
        self._block: Optional[Tensor] = None          # float64[RN_CLIP_STATE] on the device of the first gradient (kept for good)
        self._scratch: Optional[Tensor] = None        # float64[slots]: one partial sum per RN_CLIP_CHUNK elements of a gradient
        self._retired: List[Tensor] = []              # outgrown scratch buffers (a captured step may still write into them)

    @staticmethod
    def _check_max_norm(value) -> float:
        value = float(value)
        if not value > 0.0 or value == float("inf"):
            raise ValueError(f"max_norm must be a positive finite number, got {value}")
        if float(np.float32(value)) == 0.0 or not np.isfinite(np.float32(value)):
            raise ValueError(f"max_norm must be representable as a positive fp32 number, got {value}")
        return value

    def __repr__(self) -> str:
        return f"GradClip(max_norm={self._max_norm})"

    @staticmethod
    def coef(total, max_norm) -> float:
        """Pure-Python fp32 restatement of the coefficient (``csrc/clip.hip`` and ``clip_grad_norm_``): ``min((1 / (total + 1e-6)) *
        max_norm, 1)`` with every operation rounded to fp32 -- torch divides a scalar by a tensor as reciprocal-then-multiply -- and
        ``clamp(max=1)``'s treatment of NaN (it stays).  An infinite norm gives 0."""
        with np.errstate(all="ignore"):
            t = np.float32(total) + np.float32(1e-6)
            c = np.float32(np.float32(1.0) / t) * np.float32(max_norm)
            return float(np.float32(1.0) if c > np.float32(1.0) else c)

    # -- the device side ----------------------------------------------------------------------------------------------
    @property
    def max_norm(self) -> float:
        return self._max_norm

    @max_norm.setter
    def max_norm(self, value: float) -> None:
        "A new threshold: written into the device block (no re-capture needed; not inside a capture)."
        value = self._check_max_norm(value)
        if self._block is not None:
            if _is_capturing():
                raise RuntimeError("GradClip: max_norm cannot be set inside a capture (the write would replay the value of capture time)")
            self._write_max_norm(value)
        self._max_norm = value

    def _write_max_norm(self, value: float) -> None:
        dev = self._block.device
        with torch.cuda.device(dev):
            check(lib.rn_grad_clip_set(self._block.data_ptr(), float(value), torch.cuda.current_stream(dev).cuda_stream), "rn_grad_clip_set")

    def _ensure(self, device: torch.device, slots: int) -> None:
        new = self._block is None
        self._block = _device_block(self._block, RN_CLIP_STATE, device,
                                    "GradClip: take one step before capturing one: its device block cannot be created inside a capture",
                                    "GradClip: its state lives on {have}, not {want}; use one object per device")
        if new:
            self._write_max_norm(self._max_norm)
        if self._scratch is None or self._scratch.numel() < slots:
            if _is_capturing():
                raise RuntimeError("GradClip: the set of gradients grew since the last eager step: take one step before capturing one")
            if self._scratch is not None:
                self._retired.append(self._scratch)
            self._scratch = torch.empty(max(slots, 1), dtype=torch.float64, device=self._block.device)

    def compute(self, gptrs: List[int], p16s: List[int], ns: List[int], dtype16: int, scale: Optional[Tensor], device: torch.device) -> int:
        """One ``rn_grad_norm_clip`` call on the current stream over the gradients at ``gptrs`` (``p16s[i] != 0``: gradient i is
        16-bit, ``dtype16``); returns the device address of the coefficient for the step kernels."""
        n = len(gptrs)
        slots = sum((k + RN_CLIP_CHUNK - 1) // RN_CLIP_CHUNK for k in ns)
        self._ensure(device, slots)
        with torch.cuda.device(self._block.device):
            check(lib.rn_grad_norm_clip(_ptrs(gptrs), _ptrs(p16s), (C.c_int64 * n)(*ns), n, 1, dtype16,
                                        scale.data_ptr() if scale is not None else None, self._scratch.data_ptr(), self._scratch.numel(),
                                        self._block.data_ptr(), torch.cuda.current_stream().cuda_stream), "rn_grad_norm_clip")
        return self._block.data_ptr() + _CLIP_COEF_BYTE

    def _f32(self, i: int) -> Tensor:
        if self._block is None:
            raise RuntimeError("GradClip: no step has been taken yet (the device block is created by the first one)")
        return self._block.view(torch.float32)[i]

    @property
    def total_norm(self) -> Tensor:
        "The last step's global norm of the unscaled gradients (device scalar, a view into the block)."
        return self._f32(1)

    @property
    def clip_coef(self) -> Tensor:
        "The last step's coefficient, ``min(max_norm / (total_norm + 1e-6), 1)`` (device scalar, a view into the block)."
        return self._f32(2)

    def stats(self) -> Dict[str, int]:
        "Calls so far, calls that clipped (coefficient < 1) and calls with a non-finite norm (reads the block: synchronises)."
        if self._block is None:
            return {"calls": 0, "clipped": 0, "nonfinite": 0}
        calls, clipped, nonfinite = self._block.view(torch.int64)[2:5].tolist()
        return {"calls": calls, "clipped": clipped, "nonfinite": nonfinite}


RN_ACCUM_STATE = 8                      # doubles in the accumulation block (include/retinanet_hip.h)
_ACCUM_FOUND_INF = 3                    # found_inf's index among the block's 32-bit words (byte 12)


def check_accumulate_grad_batches(value, what: str = "accumulate_grad_batches") -> int:
    "``value`` as a window length: an int >= 1 (Lightning's ``accumulate_grad_batches``); dict schedules and anything else are refused."
    if isinstance(value, dict):
        raise ValueError(f"{what}: dict schedules ({{epoch: batches}}) are not supported, pass one int >= 1 (got {value!r})")
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or int(value) < 1:
        raise ValueError(f"{what} must be an int >= 1, got {value!r}")
    if int(value) >= 1 << 24:
        raise ValueError(f"{what} must be below 2**24, got {value!r}")
    return int(value)


class GradAccumulator:
    """Gradient accumulation over ``n`` micro-batches for ``MasterSGD`` / ``MasterAdam`` / ``MasterAdamW`` -- Lightning's
    ``accumulate_grad_batches`` -- into fp32 accumulators: after every backward pass ``accumulate(params)`` adds ``float(p.grad) *
    float(1 / n)`` to the parameter's accumulator (one ``rn_grad_accumulate`` call over all of them, ``csrc/accum.hip``; the first
    micro-batch of a window overwrites, so nothing is ever zeroed) and ``advance(final)`` moves the window on; the final step of a
    window hands ``grad_views()`` to ``optimizer.step(grads=...)`` first.  The 16-bit gradients of the conv weights are widened before
    they are added: autograd's own ``.grad +=`` would sum them in bf16 / fp16.

        for i, batch in enumerate(batches):
            optimizer.zero_grad(set_to_none=True); loss(batch).backward()
            acc.accumulate(net.parameters())
            final = acc.next_is_final()                  # or the caller's own rule (the last batch of an epoch)
            if final:
                optimizer.step(grads=acc.grad_views())   # (fp16: scaler.step_exchanged(optimizer, acc); scaler.update())
            acc.advance(final)

    The window position, ``float(1 / n)`` and ``found_inf`` live in a device block that the kernels read: a captured micro step is the
    same graph at every position, and assigning ``n`` (between windows only) is one tiny launch, no re-capture.  ``found_inf()`` is
    the block's flag -- 1.0 once any micro-batch of the window held a non-finite gradient element, cleared by the final ``advance`` --
    and with ``grad_views()`` makes this object what ``parallel.ExchangeGradScaler.step_exchanged`` takes in place of a gradient
    exchange: the step is skipped and the scale backs off when ANY micro-batch of the window overflowed.  The accumulators and the
    block are created by the first ``accumulate`` -- not inside a capture -- and kept for good (captured steps hold their addresses).
    ``position`` / ``stats()`` read the block (they synchronise)."""

    def __init__(self, n: int = 1):
        self._n = check_accumulate_grad_batches(n, "GradAccumulator: n")
        self._block: Optional[Tensor] = None          # float64[RN_ACCUM_STATE] on the device of the first gradient (kept for good)
        self._acc: Dict[Tensor, Tensor] = {}          # parameter -> its fp32 accumulator (the master's / parameter's strides)
        self._host_pos = 0                            # the host's mirror of the window position (micro steps since the last final one)

    def __repr__(self) -> str:
        return f"GradAccumulator(n={self._n})"

    # -- the device block ---------------------------------------------------------------------------------------------
    @property
    def n(self) -> int:
        return self._n

    @n.setter
    def n(self, value: int) -> None:
        "A new window length: written into the device block (no re-capture needed); between windows only, not inside a capture."
        value = check_accumulate_grad_batches(value, "GradAccumulator: n")
        if self._host_pos != 0:
            raise RuntimeError(f"GradAccumulator: n cannot change in mid-window ({self._host_pos} micro-batch(es) of the current window "
                               f"are already weighted 1 / {self._n}); finish the window with a final step first")
        if self._block is not None:
            if _is_capturing():
                raise RuntimeError("GradAccumulator: n cannot be set inside a capture (the write would replay the value of capture time)")
            self._write_n(value)
        self._n = value

    def _write_n(self, value: int) -> None:
        dev = self._block.device
        with torch.cuda.device(dev):
            check(lib.rn_grad_accum_set(self._block.data_ptr(), int(value), torch.cuda.current_stream(dev).cuda_stream), "rn_grad_accum_set")

    def _ensure_block(self, device: torch.device) -> None:
        new = self._block is None
        self._block = _device_block(self._block, RN_ACCUM_STATE, device,
                                    "GradAccumulator: take one step before capturing one: its device block cannot be created inside a capture",
                                    "GradAccumulator: its state lives on {have}, not {want}; use one object per device")
        if new:
            self._write_n(self._n)

    # -- the window -------------------------------------------------------------------------------------------------
    def next_is_final(self) -> bool:
        "Whether the micro-batch about to be accumulated completes the window (the host's count of the steps since the last final one)."
        return self._host_pos + 1 >= self._n

    def note_step(self, final: bool) -> None:
        "Advance the host's mirror of the window position (``advance`` does it for eager steps, ``graph.CapturedTrainStep`` for replays)."
        self._host_pos = 0 if final else self._host_pos + 1

    @torch.no_grad()
    def accumulate(self, params: Iterable[Tensor]) -> int:
        """One ``rn_grad_accumulate`` call on the current stream over every parameter of ``params`` that has a ``.grad``; returns the
        number of gradients added.  A parameter met for the first time gets its accumulator here (not inside a capture)."""
        r = _collect(params, None, self._refuse, self._accumulator, accs=[])
        if r is None:
            return 0
        self._ensure_block(r["dev"])
        n = len(r["accs"])
        with torch.cuda.device(self._block.device):
            check(lib.rn_grad_accumulate(_ptrs(r["accs"]), _ptrs(r["gptrs"]), _ptrs(r["p16s"]), (C.c_int64 * n)(*r["ns"]), n, int(bool(r["grads16"])),
                                         _dt16(r["dt16"]), self._block.data_ptr(), torch.cuda.current_stream().cuda_stream), "rn_grad_accumulate")
        return n

    @staticmethod
    def _refuse(cpu: bool) -> Exception:
        if cpu:
            return RuntimeError("GradAccumulator has no CPU fallback: it accumulates CUDA gradients (SimpleTrainer accumulates into "
                                ".grad for every other device)")
        return TypeError("GradAccumulator handles CUDA fp32 parameters and 16-bit parameters converted by use_16bit_conv_weights")

    def _accumulator(self, rec: dict, p: Tensor, w: Optional[Tensor]) -> None:
        "``_collect``'s hook: the accumulator of ``p``, created the first time it is met (not inside a capture)."
        if w is None:
            return
        a = self._acc.get(p)
        if a is None:
            if _is_capturing():
                raise RuntimeError("GradAccumulator: take one step before capturing one: the accumulators cannot be created inside a capture")
            a = self._acc[p] = torch.empty_like(w)              # the master's strides; overwritten by the window's first micro-batch
            if self._host_pos != 0:
                a.fill_(0)                                      # (a parameter that joins in mid-window starts from zero)
        rec["accs"].append(a.data_ptr())

    def advance(self, final: bool) -> None:
        """One ``rn_grad_accum_advance`` launch on the current stream, after ``accumulate`` (and, for a final step, after the optimizer
        and the scaler): a micro step moves the position on; a final one counts the window, resets the position and clears found_inf."""
        if self._block is None:
            raise RuntimeError("GradAccumulator: nothing has been accumulated yet (the device block is created by the first accumulate)")
        with torch.cuda.device(self._block.device):
            check(lib.rn_grad_accum_advance(self._block.data_ptr(), int(bool(final)), torch.cuda.current_stream().cuda_stream),
                  "rn_grad_accum_advance")
        if not _is_capturing():                       # (a captured launch runs at its replays: CapturedTrainStep notes those)
            self.note_step(final)

    def grad_views(self) -> Dict[Tensor, Tensor]:
        "``{parameter: its fp32 accumulator}`` -- what ``optimizer.step(grads=...)`` of the master optimizers consumes."
        return dict(self._acc)

    def found_inf(self) -> Tensor:
        "The window's flag (device fp32 scalar, a view into the block): 1.0 once a non-finite gradient element was accumulated, else 0."
        if self._block is None:
            raise RuntimeError("GradAccumulator: nothing has been accumulated yet (the device block is created by the first accumulate)")
        return self._block.view(torch.float32)[_ACCUM_FOUND_INF]

    @property
    def position(self) -> int:
        "The window position on the device: micro-batches accumulated since the last final step (reads the block: synchronises)."
        return 0 if self._block is None else int(self._block.view(torch.int32)[2])

    def stats(self) -> Dict[str, int]:
        "Windows completed, windows that saw a non-finite gradient, and micro-batches accumulated (reads the block: synchronises)."
        if self._block is None:
            return {"windows": 0, "nonfinite": 0, "micro_batches": 0}
        windows, nonfinite, micro = self._block.view(torch.int64)[2:5].tolist()
        return {"windows": windows, "nonfinite": nonfinite, "micro_batches": micro}


def _is_dense(t: Tensor) -> bool:
    "Whether ``t``'s elements are exactly ``numel()`` consecutive elements of memory, in whatever order of dimensions."
    expected = 1
    for size, stride in sorted(((n, st) for n, st in zip(t.shape, t.stride()) if n != 1), key=lambda x: x[1]):
        if stride != expected:
            return False
        expected *= size
    return True


RN_EMA_STATE = 8                        # doubles in the EMA block (include/retinanet_hip.h)
_EMA_OM = 8                             # om's index among the block's 32-bit words (byte 32)


class WeightEMA:
    """An exponential moving average of the fp32 weights of ``MasterSGD`` / ``MasterAdam`` / ``MasterAdamW`` -- ``--model-ema`` of
    torchvision's detection recipes, timm's ``ModelEma``, Lightning's EMA callbacks -- to be evaluated and checkpointed in place of the
    raw weights.  Install it as ``optimizer.weight_ema``: every ``step()`` then ends with ``update(all parameters, found_inf)``, one
    ``rn_ema_update`` call over the masters (``p.master`` behind a 16-bit working copy, ``p.data`` otherwise; ``csrc/ema.hip``) and one
    ``rn_ema_advance`` launch:

        ema = w                              at the first update (the average is overwritten: nothing initialises it)
        ema = ema + (w - ema) * om           afterwards, in fp32, three roundings
        om  = float32(1 - d_t),  d_t = min(decay, (1 + t) / (warmup + t)) if warmup > 0 else decay     (t: updates so far; in double)

    ``om``, the update count, ``decay`` and ``warmup`` live in a device block that the kernels read and advance: a captured step is the
    same graph at every update, and assigning ``decay`` / ``warmup`` (between replays) is one tiny launch, no re-capture.  A step that a
    loss scaler skips (``found_inf``) leaves the average and the count untouched and is counted in ``stats()["skipped"]``.  Because the
    update sits inside ``optimizer.step``, accumulation micro steps do not update, and under data parallelism every rank computes the
    same average from the same exchanged step.  The averages and the block are created by the first ``update`` -- not inside a capture --
    and kept for good (captured steps hold their addresses).

    ``swap(params)`` exchanges the training weights and the average in place, all of them at once (``rn_ema_swap``; the 16-bit working copies are refreshed
    from the new masters), ``swapped(params)`` does so around a ``with`` block: inside it the model IS the averaged model, and
    ``master_state_dict(model)`` is its checkpoint.  ``update`` raises while swapped.

    Only parameters are averaged.  BatchNorm running statistics and other buffers are NOT: the swapped model uses the live buffers
    (the reference trains with ``freeze_bn: true``, where they never move)."""

    def __init__(self, decay: float = 0.9998, warmup: float = 0.0):
        self._decay, self._warmup = self._check(decay, warmup)
        self._block: Optional[Tensor] = None          # float64[RN_EMA_STATE] on the device of the first parameter (kept for good)
        self._ema: Dict[Tensor, Tensor] = {}          # parameter -> its fp32 average (the master's / parameter's strides), in the order met
        self._swapped = False
        # A load_state_dict() into an object without averages waits here for the first update: {"updates", "ema": tensors by position}.
        # Invariant: it is only ever set while _ema is empty, the k-th average CREATED by that first update takes ema[k] (k = len(_ema)
        # at that moment, shape-checked; parameters beyond the list start from their weights), and the update drops it when it is
        # done -- a later update never sees a stale or half-consumed list.
        self._loaded: Optional[dict] = None

    @staticmethod
    def _check(decay, warmup):
        decay, warmup = float(decay), float(warmup)
        if not 0.0 <= decay < 1.0:
            raise ValueError(f"WeightEMA: decay must be in [0, 1), got {decay}")
        if not 0.0 <= warmup < float("inf"):
            raise ValueError(f"WeightEMA: warmup must be a finite number >= 0 (0 = no warm-up), got {warmup}")
        return decay, warmup

    def __repr__(self) -> str:
        return f"WeightEMA(decay={self._decay}, warmup={self._warmup})"

    @staticmethod
    def one_minus_decay(t: int, decay: float, warmup: float = 0.0) -> np.float32:
        """Pure-Python restatement of the factor of update number ``t`` (``csrc/ema.hip``): in double, ``d_t = min(decay, (1 + t) /
        (warmup + t))`` with a warm-up and ``decay`` without, then ``float32(1 - d_t)``."""
        t, decay, warmup = float(int(t)), float(decay), float(warmup)
        d = min(decay, (1.0 + t) / (warmup + t)) if warmup > 0.0 else decay
        return np.float32(1.0 - d)

    # -- the device block ---------------------------------------------------------------------------------------------
    @property
    def decay(self) -> float:
        return self._decay

    @decay.setter
    def decay(self, value: float) -> None:
        "A new decay: written into the device block (no re-capture needed; not inside a capture)."
        self._rewrite(*self._check(value, self._warmup))

    @property
    def warmup(self) -> float:
        return self._warmup

    @warmup.setter
    def warmup(self, value: float) -> None:
        "A new warm-up constant: written into the device block (no re-capture needed; not inside a capture)."
        self._rewrite(*self._check(self._decay, value))

    def _rewrite(self, decay: float, warmup: float) -> None:
        if self._block is not None:
            if _is_capturing():
                raise RuntimeError("WeightEMA: decay / warmup cannot be set inside a capture (the write would replay the values of capture time)")
            self._write(decay, warmup, -1)
        self._decay, self._warmup = decay, warmup

    def _write(self, decay: float, warmup: float, updates: int) -> None:
        dev = self._block.device
        with torch.cuda.device(dev):
            check(lib.rn_ema_set(self._block.data_ptr(), float(decay), float(warmup), int(updates), torch.cuda.current_stream(dev).cuda_stream),
                  "rn_ema_set")

    def _ensure_block(self, device: torch.device) -> None:
        new = self._block is None
        self._block = _device_block(self._block, RN_EMA_STATE, device,
                                    "WeightEMA: take one step before capturing one: its device block cannot be created inside a capture",
                                    "WeightEMA: its state lives on {have}, not {want}; use one object per device")
        if new:
            self._write(self._decay, self._warmup, self._loaded["updates"] if self._loaded is not None else 0)

    # -- the update ---------------------------------------------------------------------------------------------------
    @staticmethod
    def _refuse(cpu: bool) -> Exception:
        if cpu:
            return RuntimeError("WeightEMA has no CPU fallback: it averages the CUDA fp32 weights of MasterSGD / MasterAdam / MasterAdamW")
        return TypeError("WeightEMA handles CUDA fp32 parameters and 16-bit parameters converted by use_16bit_conv_weights")

    def _walk(self, params: Iterable[Tensor], create: bool) -> Optional[dict]:
        "One walk over ``params``: the fp32 tensor of each, its average (created here when ``create``), its 16-bit copy, the checks."
        rec = dict(emas=[], masters=[], p16s=[], ns=[], dt16=None, dev=None)
        for p in params:
            has16 = hasattr(p, "master")
            w = p.master if has16 else p.data
            if not w.is_cuda:
                raise self._refuse(True)
            if w.dtype != torch.float32:
                raise self._refuse(False)
            if rec["dev"] is None:
                rec["dev"] = w.device
            elif rec["dev"] != w.device:
                raise RuntimeError("WeightEMA: the parameters of one call must live on one device")
            # the kernels walk numel() consecutive elements from data_ptr(): a strided view would be read and written outside itself
            if not _is_dense(w) or (has16 and p.data.stride() != w.stride()):
                raise ValueError(f"WeightEMA: a parameter of shape {tuple(w.shape)} and strides {tuple(w.stride())} is not dense in memory "
                                 "(or its 16-bit copy is laid out differently): make it contiguous first")
            a = self._ema.get(p)
            if a is None:
                if not create:
                    raise RuntimeError("WeightEMA: a parameter without an average (update() has never seen it) cannot be swapped")
                if _is_capturing():
                    raise RuntimeError("WeightEMA: take one step before capturing one: the averages cannot be created inside a capture")
                a = torch.empty_like(w)                        # the master's strides
                saved = self._loaded["ema"][len(self._ema)] if self._loaded is not None and len(self._ema) < len(self._loaded["ema"]) else None
                if saved is not None and tuple(saved.shape) != tuple(w.shape):
                    raise RuntimeError(f"WeightEMA: the loaded average at position {len(self._ema)} has shape {tuple(saved.shape)}, "
                                       f"the parameter {tuple(w.shape)}")
                a.copy_(w if saved is None else saved)          # (a parameter that joins later starts from its current value)
                self._ema[p] = a
            if has16:
                if rec["dt16"] is None:
                    rec["dt16"] = p.dtype
                elif rec["dt16"] != p.dtype:
                    raise RuntimeError("the 16-bit working copies of one launch must share a dtype")
            rec["emas"].append(a.data_ptr()); rec["masters"].append(w.data_ptr()); rec["p16s"].append(p.data.data_ptr() if has16 else 0)
            rec["ns"].append(w.numel())
        return rec if rec["ns"] else None

    @torch.no_grad()
    def update(self, params: Iterable[Tensor], found_inf: Optional[Tensor] = None) -> int:
        """One ``rn_ema_update`` call and one ``rn_ema_advance`` launch on the current stream over ``params``; returns the number of
        tensors.  ``found_inf``: the loss scaler's device flag (CUDA fp32 scalar) or None; a non-zero flag skips the update on the
        device.  A parameter met for the first time gets its average here (not inside a capture)."""
        if self._swapped:
            raise RuntimeError("WeightEMA: update() while swapped would average the average: swap back first")
        if found_inf is not None and not (found_inf.is_cuda and found_inf.dtype == torch.float32 and found_inf.numel() == 1):
            raise TypeError("found_inf must be a CUDA fp32 scalar (torch.amp.GradScaler)")
        r = self._walk(params, create=True)
        if r is None:
            return 0
        self._ensure_block(r["dev"])
        self._loaded = None
        n = len(r["ns"])
        found = found_inf.data_ptr() if found_inf is not None else None
        with torch.cuda.device(self._block.device):
            stream = torch.cuda.current_stream().cuda_stream
            check(lib.rn_ema_update(_ptrs(r["emas"]), _ptrs(r["masters"]), (C.c_int64 * n)(*r["ns"]), n, self._block.data_ptr(), found, stream),
                  "rn_ema_update")
            check(lib.rn_ema_advance(self._block.data_ptr(), found, stream), "rn_ema_advance")
        return n

    # -- the swap -----------------------------------------------------------------------------------------------------
    @property
    def is_swapped(self) -> bool:
        "Whether the parameters currently hold the average (and this object the training weights)."
        return self._swapped

    @property
    def ready(self) -> bool:
        "Whether an update has created the averages (there is something to swap)."
        return bool(self._ema)

    def parameters(self) -> List[Tensor]:
        "The averaged parameters, in the order ``update`` met them."
        return list(self._ema)

    def average_of(self, p: Tensor) -> Tensor:
        "The fp32 average of parameter ``p`` (the tensor itself, not a copy; while swapped it holds the training weights)."
        a = self._ema.get(p)
        if a is None:
            raise KeyError("WeightEMA: this parameter has no average (update() has never seen it)")
        return a

    def preallocate(self, p: Tensor, storage: Tensor) -> None:
        """Keep the average of ``p`` in ``storage`` -- a CUDA fp32 tensor of the master's shape and strides, 16-byte aligned -- instead of
        allocating one (averages carved from one buffer, say).  Before ``p``'s first update only; the first update overwrites it."""
        w = p.master if hasattr(p, "master") else p.data
        if p in self._ema:
            raise RuntimeError("WeightEMA: this parameter already has its average")
        if self._loaded is not None:
            raise RuntimeError("WeightEMA: a loaded state is waiting for the first update, which hands it out by position")
        if not (storage.is_cuda and storage.dtype == torch.float32 and storage.shape == w.shape and storage.stride() == w.stride()
                and storage.device == w.device and storage.data_ptr() % 16 == 0):
            raise ValueError("WeightEMA: the storage of an average is a 16-byte aligned CUDA fp32 tensor of the master's shape, strides and device")
        self._ema[p] = storage

    @torch.no_grad()
    def swap(self, params: Optional[Iterable[Tensor]] = None) -> None:
        """Exchange the fp32 weights of every averaged parameter with their averages, in place, and refresh the 16-bit working copies
        from the new weights: one ``rn_ema_swap`` call.  A second call undoes the first bit for bit.  ``params`` (default: the averaged
        parameters) names whose weights the caller expects to change -- a model's parameters, say --: it must be exactly the averaged
        set, in any order; a subset is refused, since ``is_swapped`` is one flag for all of them."""
        if _is_capturing():
            raise RuntimeError("WeightEMA: swap() is not part of a step: it cannot be captured")
        params = self.parameters() if params is None else list(params)
        if not self._ema or not params:
            raise RuntimeError("WeightEMA: nothing to swap (the averages are created by the first update)")
        r = self._walk(params, create=False)                 # (raises for a parameter without an average)
        if len({id(p) for p in params}) != len(params) or len(params) != len(self._ema):
            raise RuntimeError(f"WeightEMA: swap() exchanges all {len(self._ema)} averaged parameters at once, got {len(params)} "
                               "(a subset would leave is_swapped meaningless)")
        n = len(r["ns"])
        with torch.cuda.device(r["dev"]):
            check(lib.rn_ema_swap(_ptrs(r["emas"]), _ptrs(r["masters"]), _ptrs(r["p16s"]), (C.c_int64 * n)(*r["ns"]), n, _dt16(r["dt16"]),
                                  torch.cuda.current_stream().cuda_stream), "rn_ema_swap")
        self._swapped = not self._swapped
        note_raw_write()                   # masters, 16-bit copies and BN affine parameters changed without a _version bump
        from . import biasact
        biasact.invalidate_dgrad_weights()

    @contextlib.contextmanager
    def swapped(self, params: Optional[Iterable[Tensor]] = None):
        "``with ema.swapped(params):`` -- the parameters hold the average inside the block and the training weights again after it."
        params = self.parameters() if params is None else list(params)
        self.swap(params)
        try:
            yield self
        finally:
            self.swap(params)

    # -- reading it back ----------------------------------------------------------------------------------------------
    @property
    def updates(self) -> int:
        "Updates applied so far, skipped steps not counted (reads the block: synchronises)."
        if self._block is None:
            return int(self._loaded["updates"]) if self._loaded is not None else 0
        return int(self._block.view(torch.int64)[2])

    def stats(self) -> Dict[str, int]:
        "Updates applied and steps skipped by found_inf (reads the block: synchronises)."
        if self._block is None:
            return {"updates": self.updates, "skipped": 0}
        updates, skipped = self._block.view(torch.int64)[2:4].tolist()
        return {"updates": updates, "skipped": skipped}

    @property
    def next_factor(self) -> Tensor:
        "``om`` of the next update (device fp32 scalar, a view into the block)."
        if self._block is None:
            raise RuntimeError("WeightEMA: no update has been made yet (the device block is created by the first one)")
        return self._block.view(torch.float32)[_EMA_OM]

    def state_dict(self) -> dict:
        "The averages by position (the order ``update`` met the parameters), ``decay``, ``warmup`` and ``updates`` (synchronises)."
        if self._swapped:
            raise RuntimeError("WeightEMA: state_dict() while swapped would save the training weights as the average: swap back first")
        if self._loaded is not None and not self._ema:
            return {"decay": self._decay, "warmup": self._warmup, "updates": self.updates, "ema": [t.clone() for t in self._loaded["ema"]]}
        return {"decay": self._decay, "warmup": self._warmup, "updates": self.updates, "ema": [a.detach().clone() for a in self._ema.values()]}

    @torch.no_grad()
    def load_state_dict(self, state: dict) -> None:
        """Restore ``decay``, ``warmup``, ``updates`` (through ``rn_ema_set``) and the averages.  Into an object that has averages they
        are copied by position; into a fresh one they wait for the first ``update``, which hands them to the parameters in its order."""
        if self._swapped:
            raise RuntimeError("WeightEMA: load_state_dict() while swapped: swap back first")
        if _is_capturing():
            raise RuntimeError("WeightEMA: load_state_dict() cannot be captured")
        decay, warmup = self._check(state["decay"], state["warmup"])
        updates, saved = int(state["updates"]), list(state["ema"])
        if updates < 0:
            raise ValueError(f"WeightEMA: updates must be >= 0, got {updates}")
        if self._ema:
            if len(saved) != len(self._ema):
                raise RuntimeError(f"WeightEMA: the state holds {len(saved)} averages, this object {len(self._ema)}")
            for a, t in zip(self._ema.values(), saved):
                if tuple(a.shape) != tuple(t.shape):
                    raise RuntimeError(f"WeightEMA: a loaded average has shape {tuple(t.shape)}, the parameter {tuple(a.shape)}")
            for a, t in zip(self._ema.values(), saved):
                a.copy_(t)
        else:
            self._loaded = {"updates": updates, "ema": [t.detach().clone() for t in saved]}
        self._decay, self._warmup = decay, warmup
        if self._block is not None:
            self._write(decay, warmup, updates)


def _amp_scalars(opt):
    "``grad_scale`` / ``found_inf`` as torch.amp.GradScaler.step sets them around the call (or None, None)."
    scale, found = getattr(opt, "grad_scale", None), getattr(opt, "found_inf", None)
    for t in (scale, found):
        if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.numel() == 1):
            raise TypeError("grad_scale / found_inf must be CUDA fp32 scalars (torch.amp.GradScaler)")
    return scale, found


def _clip_coef_ptr(opt, recs: List[dict], scale: Optional[Tensor]) -> Optional[int]:
    """With ``opt.grad_clip`` installed: the norm of the gradients of every group in ``recs`` (one call: the norm is global) and the
    device address of the coefficient; None without a clip."""
    clip = getattr(opt, "grad_clip", None)
    if clip is None or not recs:
        return None
    if not isinstance(clip, GradClip):
        raise TypeError(f"grad_clip must be an optim.GradClip, not {type(clip).__name__}")
    dt16s = {r["dt16"] for r in recs if r["dt16"] is not None}
    if len(dt16s) > 1:
        raise RuntimeError("the 16-bit working copies of a clipped step must share a dtype")
    gptrs, is16, ns = [], [], []
    for r in recs:
        gptrs += r["gptrs"]; ns += r["ns"]
        is16 += [p if r["grads16"] else 0 for p in r["p16s"]]      # (a group may hold fp32 gradients for its 16-bit copies: the exchange's views)
    return clip.compute(gptrs, is16, ns, _dt16(dt16s.pop() if dt16s else None), scale, recs[0]["dev"])


def _install_clip(opt, max_grad_norm) -> None:
    opt.grad_clip = GradClip(max_grad_norm) if max_grad_norm is not None else None


class _MasterOptimizer(torch.optim.Optimizer):
    """What ``MasterSGD`` and ``MasterAdam`` / ``MasterAdamW`` share: ``step()`` around one ``_launch`` per parameter group."""
    # torch.amp.GradScaler.step() hands such an optimizer `grad_scale` / `found_inf` (device scalars) instead of unscaling the gradients
    # and reading found_inf back on the host: the kernel divides and skips on the device, nothing synchronises
    _step_supports_amp_scaling = True
    # fp32 masters behind 16-bit conv weights (RetinaNetModel.configure_optimizers converts the model), and step(grads=...) takes the
    # fp32 bucket views of parallel.BucketedGradAllReduce
    _rn_master_weights = True
    # step() clips by global norm when `grad_clip` holds an optim.GradClip (constructor: max_grad_norm=...)
    _rn_grad_clip = True
    # step() ends with the update of `weight_ema` when that holds an optim.WeightEMA (skipped with the step on found_inf)
    _rn_weight_ema = True
    weight_ema = None
    _handles = "CUDA fp32 parameters and 16-bit parameters converted by use_16bit_conv_weights"

    @torch.no_grad()
    def step(self, closure=None, grads: Optional[Dict[Tensor, Tensor]] = None):
        """``grads``: optional ``{param: fp32 gradient}`` overriding ``param.grad`` (the fp32 views of
        ``parallel.BucketedGradAllReduce`` after the exchange, the accumulators of ``GradAccumulator``)."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._before_collect()
        note_raw_write()                   # masters, 16-bit copies and BN affine parameters change without a _version bump
        recs = [r for r in (_collect(group["params"], grads, self._refuse, self._state, gi=gi, group=group)
                            for gi, group in enumerate(self.param_groups)) if r is not None]
        scale, found = _amp_scalars(self)                                  # (set by GradScaler.step around this call)
        coef = _clip_coef_ptr(self, recs, scale)                           # (None without a clip: the unclipped step)
        for r in recs:
            with torch.cuda.device(r["dev"]):
                self._launch(r, scale.data_ptr() if scale is not None else None, found.data_ptr() if found is not None else None, coef)
        ema = getattr(self, "weight_ema", None)
        if ema is not None and recs:
            if not isinstance(ema, WeightEMA):
                raise TypeError(f"weight_ema must be an optim.WeightEMA, not {type(ema).__name__}")
            ema.update((p for group in self.param_groups for p in group["params"]), found)
        from . import biasact
        biasact.invalidate_dgrad_weights()           # (the kernel wrote the parameters through raw pointers: no version counter moved)
        return loss

    def _refuse(self, cpu: bool) -> Exception:
        return TypeError(f"{type(self).__name__} handles {self._handles}")

    def _before_collect(self) -> None:
        pass

    def _state(self, rec: dict, p: Tensor, w: Optional[Tensor]) -> None:
        "``_collect``'s hook: create the state of ``p`` (``w``: its fp32 tensor; None: ``p`` has no gradient) and add its pointers to ``rec``."
        raise NotImplementedError

    def _launch(self, rec: dict, scale: Optional[int], found: Optional[int], coef: Optional[int]) -> None:
        "The step of one group's ``rec`` on the current stream (``scale`` / ``found`` / ``coef``: nullable device addresses)."
        raise NotImplementedError


RN_SGD_HPARAMS = 8                      # 32-bit words per group in MasterSGD's device block (include/retinanet_hip.h)
_SHP_STEPS = 5                          # the step counter's word in it


class MasterSGD(_MasterOptimizer):
    """``torch.optim.SGD`` on fp32 masters with 16-bit conv working copies, one HIP launch per 48 tensors and parameter group.

    By default lr, momentum, dampening, weight_decay, nesterov and "this is the first step" go to ``rn_sgd_master_step`` by value: they
    are part of a captured graph's key, and the host counts the steps.

    ``capturable=True``: the same update through ``rn_sgd_master_step_dev`` -- bit for bit at equal hyperparameters -- with those values
    and the step count in a device block per group that the kernels read, so a step captured in a graph follows whatever the host
    wrote last.  ``sync_device_hparams()`` writes each group's current values there (``step()`` calls it when the stream is not
    capturing; ``graph.CapturedTrainStep`` calls it before every replay): a per-step LR schedule keeps replaying one graph.  The step
    count advances on the device, and not at all in a step that ``torch.amp.GradScaler`` skips (found_inf), so a skipped first step
    stays first and ``dampening != 0`` works under loss scaling.  What decides which memory exists is fixed once a group's block
    exists -- whether it has momentum buffers (``momentum != 0`` at that time) and ``nesterov``; changing either raises a
    ``ValueError``.  lr, dampening, weight_decay and momentum (any value for a group with buffers; with ``momentum == 0`` the buffer
    keeps the last gradient) are rewritable between replays.  The blocks and buffers are created by the first step -- not inside a
    capture -- and kept for good.

    ``state_dict()`` / ``load_state_dict()`` use torch's SGD format (``momentum_buffer`` per parameter) plus ``steps``, the number of
    steps taken: checkpoints move between both modes of this class and ``torch.optim.SGD`` in every direction (torch's state with a
    ``momentum_buffer`` present loads as "not the first step"; weights: ``master_state_dict`` / ``load_master_state_dict``).  In
    capturable mode ``state_dict()`` and ``group_steps()`` read the count back from the device (they synchronise)."""
    _handles = "CUDA fp32 parameters and bf16 parameters converted by use_bf16_conv_weights"

    def __init__(self, params: Iterable, lr: float = 1e-3, momentum: float = 0.0, dampening: float = 0.0,
                 weight_decay: float = 0.0, nesterov: bool = False, max_grad_norm: Optional[float] = None, *, capturable: bool = False):
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        if not isinstance(capturable, (bool, np.bool_)):
            raise TypeError(f"capturable must be a bool, got {capturable!r}")
        self._capturable = bool(capturable)
        if self._capturable:
            self._check_values(lr, momentum, dampening, weight_decay)
            self._rn_device_hparams = True               # lr .. nesterov are read on the device: no part of a captured graph's key
            self._blocks: Dict[int, Tensor] = {}         # group index -> its device block (RN_SGD_HPARAMS 32-bit words)
            self._written: Dict[int, tuple] = {}         # group index -> the values last written into it
            self._structure: Dict[int, tuple] = {}       # group index -> (has momentum buffers, nesterov), fixed with the block
        _install_clip(self, max_grad_norm)
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov))

    @property
    def capturable(self) -> bool:
        return self._capturable

    # -- by value (the default) ----------------------------------------------------------------------------------
    def _state(self, rec: dict, p: Tensor, w: Optional[Tensor]) -> None:
        if self._capturable:
            return self._state_dev(rec, p, w)
        if w is None:
            return
        group, st = rec["group"], self.state[p]
        if "momentum_buffer" not in st:
            # (under a GradScaler the very first step may be SKIPPED by found_inf: the buffer then has to hold zeros, with
            # which the next step's momentum * buf + (1 - dampening) * g is torch's first-step buf = g -- for dampening == 0
            # only; a fill kernel, not a memset: graph.py)
            amp = getattr(self, "found_inf", None) is not None
            if amp and group["momentum"] != 0 and group["dampening"] != 0:
                raise ValueError("MasterSGD under loss scaling needs dampening == 0: a first step skipped by found_inf leaves a zero "
                                 "momentum buffer, and the next step's momentum * 0 + (1 - dampening) * g is not torch.optim.SGD's first-step buf = g")
            st["momentum_buffer"] = (torch.empty_like(w).fill_(0) if amp else torch.empty_like(w)) if group["momentum"] != 0 else None
            st["steps"] = 0
        if rec.setdefault("first", st["steps"] == 0) != (st["steps"] == 0):
            raise RuntimeError("parameters of one group must have taken the same number of steps")
        st["steps"] += 1
        rec.setdefault("moms", []).append(st["momentum_buffer"].data_ptr() if st["momentum_buffer"] is not None else 0)

    def _launch(self, rec: dict, scale: Optional[int], found: Optional[int], coef: Optional[int]) -> None:
        if self._capturable:
            return self._launch_dev(rec, scale, found, coef)
        group, n = rec["group"], len(rec["ns"])
        check(lib.rn_sgd_master_step(_ptrs(rec["masters"]), _ptrs(rec["moms"]), _ptrs(rec["gptrs"]), _ptrs(rec["p16s"]), (C.c_int64 * n)(*rec["ns"]), n,
                                     int(bool(rec["grads16"])), _dt16(rec["dt16"]), float(group["lr"]), float(group["momentum"]),
                                     float(group["dampening"]), float(group["weight_decay"]), int(group["nesterov"]), int(bool(rec["first"])),
                                     scale, found, coef, torch.cuda.current_stream().cuda_stream), "rn_sgd_master_step")

    # -- capturable: the device blocks ---------------------------------------------------------------------------
    @staticmethod
    def _check_values(lr, momentum, dampening, weight_decay) -> None:
        if isinstance(lr, Tensor):
            raise ValueError("MasterSGD(capturable=True): lr is a float (the device block holds it), not a Tensor")
        for name, v, lo in (("lr", lr, 0.0), ("momentum", momentum, 0.0), ("dampening", dampening, None), ("weight_decay", weight_decay, 0.0)):
            v = float(v)
            if not abs(v) <= float(np.finfo(np.float32).max) or (lo is not None and v < lo):      # (NaN fails the first test)
                raise ValueError(f"Invalid {name} value: {v} (a finite fp32 number" + (f" >= {lo})" if lo is not None else ")"))

    def _hparams(self, i: int, group) -> tuple:
        "The values of group ``i`` as the block takes them, checked: (lr, momentum, dampening, weight_decay, nesterov)."
        self._check_values(group["lr"], group["momentum"], group["dampening"], group["weight_decay"])
        vals = (float(group["lr"]), float(group["momentum"]), float(group["dampening"]), float(group["weight_decay"]), int(bool(group["nesterov"])))
        if vals[4] and (vals[1] <= 0 or vals[2] != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        fixed = self._structure.get(i)
        if fixed is not None:
            has_m, nesterov = fixed
            if bool(vals[4]) != nesterov:
                raise ValueError(f"MasterSGD(capturable=True): nesterov of parameter group {i} is fixed at {nesterov} once its device block "
                                 "exists; construct a new optimizer to change it")
            if not has_m and vals[1] != 0.0:
                raise ValueError(f"MasterSGD(capturable=True): momentum of parameter group {i} cannot become non-zero: the group started "
                                 "with momentum == 0 and has no momentum buffers; construct the optimizer with a non-zero momentum")
        return vals

    def _block(self, i: int, group, dev: torch.device) -> Tensor:
        blk = _device_block(self._blocks.get(i), RN_SGD_HPARAMS // 2, dev,
                            "MasterSGD: take one step (or call sync_device_hparams()) before capturing a step: "
                            "the device blocks and momentum buffers cannot be created inside a capture",
                            f"MasterSGD: the state of parameter group {i} lives on {{have}}, not {{want}}; a group stays on one device")
        if i not in self._blocks:
            self._blocks[i] = blk
            self._written.pop(i, None)
            self._structure[i] = (float(group["momentum"]) != 0.0, bool(group["nesterov"]))
        return blk

    def _write_block(self, i: int, group, step: int = -1) -> None:
        dev = group["params"][0].device
        vals = self._hparams(i, group)
        blk = self._block(i, group, dev)
        with torch.cuda.device(dev):
            check(lib.rn_sgd_hparams_set(blk.data_ptr(), *vals, int(step), torch.cuda.current_stream(dev).cuda_stream), "rn_sgd_hparams_set")
        self._written[i] = vals

    def sync_device_hparams(self) -> None:
        """Capturable mode: write each group's current lr / momentum / dampening / weight_decay / nesterov into its device block on the
        current stream: one small launch per group whose values changed since the last write, none otherwise.  Never synchronises;
        does nothing while the current stream is capturing (a write recorded into a graph would replay the values of capture time)
        and nothing in the default mode (no value lives on the device)."""
        if not self._capturable or _is_capturing():
            return
        for i, group in enumerate(self.param_groups):
            if not group["params"] or not group["params"][0].is_cuda:
                continue
            if i not in self._blocks or self._written.get(i) != self._hparams(i, group):
                self._write_block(i, group)

    def _before_collect(self) -> None:
        self.sync_device_hparams()                   # (does nothing by value, or while the stream is capturing)

    def _state_dev(self, rec: dict, p: Tensor, w: Optional[Tensor]) -> None:
        has_state = "momentum_buffer" in self.state.get(p, {})
        if w is None:
            if has_state:
                raise RuntimeError("MasterSGD(capturable=True): a parameter with optimizer state has no gradient in this step: the step "
                                   "counter is one per group, so every parameter of a group must step together")
            return
        st = self.state[p]
        if not has_state:
            if _is_capturing():
                raise RuntimeError("MasterSGD: take one step before capturing one: the momentum buffers cannot be created inside a capture")
            fixed = self._structure.get(rec["gi"])
            has_m = fixed[0] if fixed is not None else float(rec["group"]["momentum"]) != 0.0
            # same memory order as the master (empty_like keeps the strides); a fill kernel, not a memset (graph.py).  The first step
            # does not read it; zeros rather than garbage for a checkpoint taken after a skipped first step
            st["momentum_buffer"] = torch.empty_like(w).fill_(0) if has_m else None
        if rec.setdefault("had_state", has_state) != has_state:
            raise RuntimeError("MasterSGD(capturable=True): a parameter joined a group that has already stepped: the step counter is one per group")
        rec.setdefault("moms", []).append(st["momentum_buffer"].data_ptr() if st["momentum_buffer"] is not None else 0)

    def _launch_dev(self, rec: dict, scale: Optional[int], found: Optional[int], coef: Optional[int]) -> None:
        n = len(rec["ns"])
        blk = self._block(rec["gi"], rec["group"], rec["dev"])               # (raises under capture when it is not there yet)
        check(lib.rn_sgd_master_step_dev(_ptrs(rec["masters"]), _ptrs(rec["moms"]), _ptrs(rec["gptrs"]), _ptrs(rec["p16s"]), (C.c_int64 * n)(*rec["ns"]),
                                         n, int(bool(rec["grads16"])), _dt16(rec["dt16"]), int(self._structure[rec["gi"]][0]), blk.data_ptr(),
                                         scale, found, coef, torch.cuda.current_stream().cuda_stream), "rn_sgd_master_step_dev")

    # -- checkpoints in torch's SGD format, plus the count ---------------------------------------------------------
    def group_steps(self) -> List[int]:
        "The steps every parameter group has taken (capturable mode: reads the device blocks, which synchronises)."
        if self._capturable:
            return [int(self._blocks[i].view(torch.int32)[_SHP_STEPS]) if i in self._blocks else 0 for i in range(len(self.param_groups))]
        return [max((self.state[p].get("steps", 0) for p in g["params"] if p in self.state), default=0) for g in self.param_groups]

    def state_dict(self):
        sd = super().state_dict()
        if not self._capturable:
            return sd
        steps = self.group_steps()
        idx = 0
        for gi, group in enumerate(self.param_groups):
            for _ in group["params"]:
                st = sd["state"].get(idx)
                if st is not None:
                    sd["state"][idx] = {"momentum_buffer": st["momentum_buffer"], "steps": steps[gi]}
                idx += 1
        return sd

    def load_state_dict(self, state_dict) -> None:
        """Load a checkpoint of this class (either mode) or of ``torch.optim.SGD``: the momentum buffers are copied in fp32 into the
        masters' memory order, ``steps`` (torch's state has none: 1 where a ``momentum_buffer`` is present, else 0) into the host's
        count or the device block.  Parameters of one group must carry one count."""
        saved_state, saved_groups = state_dict["state"], state_dict["param_groups"]
        counts = []
        for g in saved_groups:
            if g.get("maximize"):
                raise ValueError("MasterSGD cannot resume a maximize=True checkpoint")
            vals = set()
            for i in g["params"]:
                if i in saved_state:
                    st = saved_state[i]
                    vals.add(int(st["steps"]) if "steps" in st else int(st.get("momentum_buffer") is not None))
            if len(vals) > 1:
                raise RuntimeError(f"MasterSGD: the parameters of one group took different numbers of steps ({sorted(vals)}): the count is one per group")
            counts.append(vals.pop() if vals else 0)
        # torch's loader restores the groups' hyperparameters; it would cast the buffers to the PARAMETER's dtype (bf16 for a
        # converted conv weight), so they are left out of it and copied below
        super().load_state_dict({"state": {}, "param_groups": saved_groups})
        idx = 0
        with torch.no_grad():
            for gi, group in enumerate(self.param_groups):
                if self._capturable:
                    self._hparams(gi, group)                                 # (a checkpoint that contradicts the fixed settings is refused)
                    fixed = self._structure.get(gi)
                    has_m = fixed[0] if fixed is not None else float(group["momentum"]) != 0.0
                else:
                    has_m = float(group["momentum"]) != 0.0
                for p in group["params"]:
                    saved = saved_state.get(idx)
                    idx += 1
                    if saved is None:
                        continue
                    buf = saved.get("momentum_buffer")
                    w = p.master if hasattr(p, "master") else p.data
                    if has_m and buf is None:
                        if self._capturable:
                            self.state[p]["momentum_buffer"] = torch.empty_like(w).fill_(0)
                        continue                                             # (by value: the next step creates the buffer, as a first step)
                    st = self.state[p]
                    st["momentum_buffer"] = torch.empty_like(w).copy_(buf) if has_m else None
                    if not self._capturable:
                        st["steps"] = counts[gi]
        if self._capturable:
            for gi, group in enumerate(self.param_groups):
                if group["params"] and group["params"][0].is_cuda:
                    self._write_block(gi, group, counts[gi])

RN_ADAM_HPARAMS = 16                    # doubles per group in the device block (include/retinanet_hip.h)
_HP_STEP = 5                            # the step counter's slot in it


class _MasterAdamBase(_MasterOptimizer):
    """``torch.optim.Adam`` / ``AdamW`` on fp32 masters with 16-bit conv working copies (``use_16bit_conv_weights``), in one HIP
    prologue plus one launch per 40 tensors and parameter group (``rn_adam_master_step``, ``csrc/adam.hip``): torch's single-tensor
    fp32 arithmetic, in its order.

    Capturable: lr, betas, eps, weight_decay and the step counter live in a device block per group that the kernels read, so a
    step captured in a graph follows whatever the host wrote last.  ``sync_device_hparams()`` writes each group's current
    hyperparameters there (``step()`` calls it when the stream is not capturing; ``graph.CapturedTrainStep`` calls it before every
    replay): an LR scheduler that changes ``lr`` every step keeps replaying one graph.  The step counter advances on the device,
    and not at all in a step that ``torch.amp.GradScaler`` skips (found_inf), as in torch's fused Adam.  ``state_dict()`` /
    ``load_state_dict()`` use torch's Adam format (per-parameter ``step``, ``exp_avg``, ``exp_avg_sq``): checkpoints move both ways
    between this class and its torch counterpart (weights: ``master_state_dict`` / ``load_master_state_dict``)."""
    _rn_device_hparams = True            # lr / betas / eps / weight_decay are read on the device: no part of a captured graph's key
    _decoupled = False

    def __init__(self, params: Iterable, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 amsgrad: bool = False, *, maximize: bool = False, max_grad_norm: Optional[float] = None):
        if isinstance(lr, Tensor) or not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr} (a float >= 0)")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        betas = tuple(float(b) for b in betas)
        if len(betas) != 2 or not all(0.0 <= b < 1.0 for b in betas):
            raise ValueError(f"Invalid betas: {betas} (two floats in [0, 1))")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if amsgrad:
            raise ValueError(f"{type(self).__name__} does not implement AMSGrad (amsgrad=True)")
        if maximize:
            raise ValueError(f"{type(self).__name__} does not implement maximize=True")
        _install_clip(self, max_grad_norm)
        self._blocks: Dict[int, Tensor] = {}         # group index -> its device block (float64[RN_ADAM_HPARAMS])
        self._written: Dict[int, tuple] = {}         # group index -> the hyperparameters last written into it
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False))

    # -- the device blocks ---------------------------------------------------------------------------------------
    @staticmethod
    def _hparams(group) -> tuple:
        b1, b2 = group["betas"]
        return (float(group["lr"]), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]))

    def _block(self, i: int, dev: torch.device) -> Tensor:
        name = type(self).__name__
        blk = _device_block(self._blocks.get(i), RN_ADAM_HPARAMS, dev,
                            f"{name}: take one step (or call sync_device_hparams()) before capturing a step: "
                            "the device blocks and moments cannot be created inside a capture",
                            f"{name}: the state of parameter group {i} lives on {{have}}, not {{want}}; a group stays on one device")
        if i not in self._blocks:
            self._blocks[i] = blk
            self._written.pop(i, None)
        return blk

    def _write_block(self, i: int, group, step: float = -1.0) -> None:
        dev = group["params"][0].device
        blk = self._block(i, dev)
        vals = self._hparams(group)
        with torch.cuda.device(dev):
            check(lib.rn_adam_hparams_set(blk.data_ptr(), *vals, float(step), torch.cuda.current_stream(dev).cuda_stream),
                  "rn_adam_hparams_set")
        self._written[i] = vals

    def sync_device_hparams(self) -> None:
        """Write each group's current lr / betas / eps / weight_decay into its device block on the current stream: one small launch
        per group whose values changed since the last write, none otherwise.  Never synchronises; does nothing while the current
        stream is capturing (a write recorded into a graph would replay the values of capture time)."""
        if _is_capturing():
            return
        for i, group in enumerate(self.param_groups):
            if not group["params"] or not group["params"][0].is_cuda:
                continue
            if self._written.get(i) != self._hparams(group) or i not in self._blocks:
                self._write_block(i, group)

    # -- the step ------------------------------------------------------------------------------------------------
    def _before_collect(self) -> None:
        self.sync_device_hparams()                   # (does nothing while the stream is capturing)

    def _state(self, rec: dict, p: Tensor, w: Optional[Tensor]) -> None:
        name = type(self).__name__
        has_state = "exp_avg" in self.state.get(p, {})
        if w is None:
            if has_state:
                raise RuntimeError(f"{name}: a parameter with optimizer state has no gradient in this step: the step counter is "
                                   "one per group, so every parameter of a group must step together")
            return
        st = self.state[p]
        if not has_state:
            if _is_capturing():
                raise RuntimeError(f"{name}: take one step before capturing one: the moments cannot be created inside a capture")
            # same memory order as the master (empty_like keeps the strides); a fill kernel, not a memset (graph.py)
            st["exp_avg"] = torch.empty_like(w).fill_(0)
            st["exp_avg_sq"] = torch.empty_like(w).fill_(0)
        if rec.setdefault("had_state", has_state) != has_state:
            raise RuntimeError(f"{name}: a parameter joined a group that has already stepped: the step counter is one per group")
        rec.setdefault("ms", []).append(st["exp_avg"].data_ptr()); rec.setdefault("vs", []).append(st["exp_avg_sq"].data_ptr())

    def _launch(self, rec: dict, scale: Optional[int], found: Optional[int], coef: Optional[int]) -> None:
        n = len(rec["ns"])
        blk = self._block(rec["gi"], rec["dev"])                             # (raises under capture when it is not there yet)
        check(lib.rn_adam_master_step(_ptrs(rec["masters"]), _ptrs(rec["ms"]), _ptrs(rec["vs"]), _ptrs(rec["gptrs"]), _ptrs(rec["p16s"]),
                                      (C.c_int64 * n)(*rec["ns"]), n, int(bool(rec["grads16"])), _dt16(rec["dt16"]), int(self._decoupled),
                                      blk.data_ptr(), scale, found, coef, torch.cuda.current_stream().cuda_stream), "rn_adam_master_step")

    # -- checkpoints in torch's Adam format ------------------------------------------------------------------------
    def group_steps(self) -> List[float]:
        "The step counter of every parameter group (reads the device blocks: synchronises)."
        return [float(self._blocks[i][_HP_STEP]) if i in self._blocks else 0.0 for i in range(len(self.param_groups))]

    def state_dict(self):
        sd = super().state_dict()
        steps = self.group_steps()
        idx = 0
        for gi, group in enumerate(self.param_groups):
            for _ in group["params"]:
                st = sd["state"].get(idx)
                if st is not None:
                    sd["state"][idx] = {"step": torch.tensor(steps[gi], dtype=torch.float32), "exp_avg": st["exp_avg"],
                                        "exp_avg_sq": st["exp_avg_sq"]}
                idx += 1
        return sd

    def load_state_dict(self, state_dict) -> None:
        """Load a checkpoint of this class or of ``torch.optim.Adam`` / ``AdamW``: the moments are copied in fp32 into the masters'
        memory order, the hyperparameters and each group's step counter into the device blocks.  Parameters of one group must carry
        one step count (the counter is per group)."""
        name = type(self).__name__
        saved_state, saved_groups = state_dict["state"], state_dict["param_groups"]
        steps = []
        for g in saved_groups:
            if g.get("amsgrad") or g.get("maximize"):
                raise ValueError(f"{name} cannot resume an AMSGrad / maximize checkpoint")
            vals = {float(saved_state[i]["step"]) for i in g["params"] if i in saved_state}
            if len(vals) > 1:
                raise RuntimeError(f"{name}: the parameters of one group took different numbers of steps ({sorted(vals)}): the step "
                                   "counter is one per group")
            steps.append(vals.pop() if vals else 0.0)
        # torch's loader restores the groups' hyperparameters; it would cast the moments to the PARAMETER's dtype (bf16 for a
        # converted conv weight), so they are left out of it and copied below
        super().load_state_dict({"state": {}, "param_groups": saved_groups})
        for g in self.param_groups:
            g["betas"] = tuple(g["betas"])
        flat = [p for g in self.param_groups for p in g["params"]]
        with torch.no_grad():
            for i, p in enumerate(flat):
                if i not in saved_state:
                    continue
                w = p.master if hasattr(p, "master") else p.data
                st = self.state[p]
                st["exp_avg"] = torch.empty_like(w).copy_(saved_state[i]["exp_avg"])
                st["exp_avg_sq"] = torch.empty_like(w).copy_(saved_state[i]["exp_avg_sq"])
        for gi, group in enumerate(self.param_groups):
            if group["params"] and group["params"][0].is_cuda:
                self._write_block(gi, group, steps[gi])


class MasterAdam(_MasterAdamBase):
    "``torch.optim.Adam`` (L2 weight decay: g += weight_decay * w) on fp32 masters, capturable: see ``_MasterAdamBase``."

    def __init__(self, params: Iterable, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 amsgrad: bool = False, *, maximize: bool = False, max_grad_norm: Optional[float] = None):
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad, maximize=maximize, max_grad_norm=max_grad_norm)


class MasterAdamW(_MasterAdamBase):
    "``torch.optim.AdamW`` (decoupled weight decay: w *= 1 - lr * weight_decay) on fp32 masters, capturable: see ``_MasterAdamBase``."
    _decoupled = True

    def __init__(self, params: Iterable, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 amsgrad: bool = False, *, maximize: bool = False, max_grad_norm: Optional[float] = None):
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad, maximize=maximize, max_grad_norm=max_grad_norm)
