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
"""
import ctypes as C
from typing import Dict, Iterable, List, Optional

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


class MasterSGD(torch.optim.Optimizer):
    # torch.amp.GradScaler.step() hands such an optimizer `grad_scale` / `found_inf` (device scalars) instead of unscaling the gradients
    # and reading found_inf back on the host: the kernel divides and skips on the device (rn_sgd_master_step_ex), nothing synchronises
    _step_supports_amp_scaling = True
    # fp32 masters behind 16-bit conv weights (RetinaNetModel.configure_optimizers converts the model), and step(grads=...) takes the
    # fp32 bucket views of parallel.BucketedGradAllReduce
    _rn_master_weights = True

    def __init__(self, params: Iterable, lr: float = 1e-3, momentum: float = 0.0, dampening: float = 0.0,
                 weight_decay: float = 0.0, nesterov: bool = False):
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov))

    @torch.no_grad()
    def step(self, closure=None, grads: Optional[Dict[Tensor, Tensor]] = None):
        """``grads``: optional ``{param: fp32 gradient}`` overriding ``param.grad`` (the fp32 views of
        ``parallel.BucketedGradAllReduce`` after the exchange)."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        note_raw_write()                   # masters, bf16 copies and BN affine parameters change without a _version bump
        for group in self.param_groups:
            masters, moms, gptrs, p16s, ns = [], [], [], [], []
            grads16 = None
            dt16 = None
            first = None
            keep: List[Tensor] = []
            for p in group["params"]:
                g = grads.get(p) if grads is not None else None
                if g is None:
                    g = p.grad
                if g is None:
                    continue
                has16 = hasattr(p, "master")
                w = p.master if has16 else p.data
                if w.dtype != torch.float32 or not p.is_cuda:
                    raise TypeError("MasterSGD handles CUDA fp32 parameters and bf16 parameters converted by use_bf16_conv_weights")
                st = self.state[p]
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
                if first is None:
                    first = st["steps"] == 0
                elif first != (st["steps"] == 0):
                    raise RuntimeError("parameters of one group must have taken the same number of steps")
                st["steps"] += 1
                if has16:
                    if dt16 is None:
                        dt16 = p.dtype
                    elif dt16 != p.dtype:
                        raise RuntimeError("the 16-bit working copies of one group must share a dtype")
                    is16 = g.dtype == p.dtype
                    if not is16 and g.dtype != torch.float32:
                        raise TypeError(f"unsupported gradient dtype {g.dtype} for a {p.dtype} working copy")
                    if grads16 is None:
                        grads16 = is16
                    elif grads16 != is16:
                        raise RuntimeError("gradients of the 16-bit parameters must be all 16-bit or all fp32")
                elif g.dtype != torch.float32:
                    raise TypeError("fp32 parameters need fp32 gradients")
                # same memory order for master / momentum / gradient / bf16 copy: all carry the parameter's strides
                if g.stride() != w.stride():
                    g = g.contiguous(memory_format=torch.channels_last) if w.dim() == 4 and w.is_contiguous(memory_format=torch.channels_last) \
                        else g.contiguous()
                    keep.append(g)
                masters.append(w.data_ptr()); moms.append(st["momentum_buffer"].data_ptr() if st["momentum_buffer"] is not None else 0)
                gptrs.append(g.data_ptr()); p16s.append(p.data.data_ptr() if has16 else 0); ns.append(w.numel())
            n = len(masters)
            if n == 0:
                continue
            dev = group["params"][0].device
            scale, found = getattr(self, "grad_scale", None), getattr(self, "found_inf", None)       # (set by GradScaler.step around this call)
            for t in (scale, found):
                if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.numel() == 1):
                    raise TypeError("grad_scale / found_inf must be CUDA fp32 scalars (torch.amp.GradScaler)")
            with torch.cuda.device(dev):
                check(lib.rn_sgd_master_step_ex((C.c_void_p * n)(*masters), (C.c_void_p * n)(*moms), (C.c_void_p * n)(*gptrs),
                                                (C.c_void_p * n)(*p16s), (C.c_int64 * n)(*ns), n, int(bool(grads16)),
                                                RN_F16 if dt16 == torch.float16 else RN_BF16, float(group["lr"]),
                                                float(group["momentum"]), float(group["dampening"]), float(group["weight_decay"]),
                                                int(group["nesterov"]), int(bool(first)), scale.data_ptr() if scale is not None else None,
                                                found.data_ptr() if found is not None else None, torch.cuda.current_stream().cuda_stream),
                      "rn_sgd_master_step_ex")
        from . import biasact
        biasact.invalidate_dgrad_weights()           # (the kernel wrote the parameters through raw pointers: no version counter moved)
        return loss


RN_ADAM_HPARAMS = 16                    # doubles per group in the device block (include/retinanet_hip.h)
_HP_STEP = 5                            # the step counter's slot in it


def _is_capturing() -> bool:
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


class _MasterAdamBase(torch.optim.Optimizer):
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
    _step_supports_amp_scaling = True
    _rn_master_weights = True
    _rn_device_hparams = True            # lr / betas / eps / weight_decay are read on the device: no part of a captured graph's key
    _decoupled = False

    def __init__(self, params: Iterable, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 amsgrad: bool = False, *, maximize: bool = False):
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
        self._blocks: Dict[int, Tensor] = {}         # group index -> its device block (float64[RN_ADAM_HPARAMS])
        self._written: Dict[int, tuple] = {}         # group index -> the hyperparameters last written into it
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False))

    # -- the device blocks ---------------------------------------------------------------------------------------
    @staticmethod
    def _hparams(group) -> tuple:
        b1, b2 = group["betas"]
        return (float(group["lr"]), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]))

    def _block(self, i: int, dev: torch.device) -> Tensor:
        blk = self._blocks.get(i)
        if blk is None:
            if _is_capturing():
                raise RuntimeError(f"{type(self).__name__}: take one step (or call sync_device_hparams()) before capturing a step: "
                                   "the device blocks and moments cannot be created inside a capture")
            blk = torch.empty(RN_ADAM_HPARAMS, dtype=torch.float64, device=dev).fill_(0)      # (a fill kernel, not a memset: graph.py)
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
    @torch.no_grad()
    def step(self, closure=None, grads: Optional[Dict[Tensor, Tensor]] = None):
        """``grads``: optional ``{param: fp32 gradient}`` overriding ``param.grad`` (the fp32 views of
        ``parallel.BucketedGradAllReduce`` after the exchange), as for ``MasterSGD``."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        capturing = _is_capturing()
        if not capturing:
            self.sync_device_hparams()
        note_raw_write()                   # masters, 16-bit copies and BN affine parameters change without a _version bump
        name = type(self).__name__
        for gi, group in enumerate(self.param_groups):
            masters, ms, vs, gptrs, p16s, ns = [], [], [], [], [], []
            grads16 = None
            dt16 = None
            keep: List[Tensor] = []
            had_state = new_state = False
            for p in group["params"]:
                g = grads.get(p) if grads is not None else None
                if g is None:
                    g = p.grad
                if g is None:
                    if "exp_avg" in self.state.get(p, {}):
                        raise RuntimeError(f"{name}: a parameter with optimizer state has no gradient in this step: the step counter is "
                                           "one per group, so every parameter of a group must step together")
                    continue
                has16 = hasattr(p, "master")
                w = p.master if has16 else p.data
                if w.dtype != torch.float32 or not p.is_cuda:
                    raise TypeError(f"{name} handles CUDA fp32 parameters and 16-bit parameters converted by use_16bit_conv_weights")
                st = self.state[p]
                if "exp_avg" not in st:
                    if capturing:
                        raise RuntimeError(f"{name}: take one step before capturing one: the moments cannot be created inside a capture")
                    # same memory order as the master (empty_like keeps the strides); a fill kernel, not a memset (graph.py)
                    st["exp_avg"] = torch.empty_like(w).fill_(0)
                    st["exp_avg_sq"] = torch.empty_like(w).fill_(0)
                    new_state = True
                else:
                    had_state = True
                if has16:
                    if dt16 is None:
                        dt16 = p.dtype
                    elif dt16 != p.dtype:
                        raise RuntimeError("the 16-bit working copies of one group must share a dtype")
                    is16 = g.dtype == p.dtype
                    if not is16 and g.dtype != torch.float32:
                        raise TypeError(f"unsupported gradient dtype {g.dtype} for a {p.dtype} working copy")
                    if grads16 is None:
                        grads16 = is16
                    elif grads16 != is16:
                        raise RuntimeError("gradients of the 16-bit parameters must be all 16-bit or all fp32")
                elif g.dtype != torch.float32:
                    raise TypeError("fp32 parameters need fp32 gradients")
                # same memory order for master / moments / gradient / 16-bit copy: all carry the parameter's strides
                if g.stride() != w.stride():
                    g = g.contiguous(memory_format=torch.channels_last) if w.dim() == 4 and w.is_contiguous(memory_format=torch.channels_last) \
                        else g.contiguous()
                    keep.append(g)
                masters.append(w.data_ptr()); ms.append(st["exp_avg"].data_ptr()); vs.append(st["exp_avg_sq"].data_ptr())
                gptrs.append(g.data_ptr()); p16s.append(p.data.data_ptr() if has16 else 0); ns.append(w.numel())
            if had_state and new_state:
                raise RuntimeError(f"{name}: a parameter joined a group that has already stepped: the step counter is one per group")
            n = len(masters)
            if n == 0:
                continue
            dev = group["params"][0].device
            blk = self._blocks.get(gi)
            if blk is None:
                blk = self._block(gi, dev)              # (raises under capture)
            scale, found = getattr(self, "grad_scale", None), getattr(self, "found_inf", None)       # (set by GradScaler.step around this call)
            for t in (scale, found):
                if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.numel() == 1):
                    raise TypeError("grad_scale / found_inf must be CUDA fp32 scalars (torch.amp.GradScaler)")
            with torch.cuda.device(dev):
                check(lib.rn_adam_master_step((C.c_void_p * n)(*masters), (C.c_void_p * n)(*ms), (C.c_void_p * n)(*vs),
                                              (C.c_void_p * n)(*gptrs), (C.c_void_p * n)(*p16s), (C.c_int64 * n)(*ns), n,
                                              int(bool(grads16)), RN_F16 if dt16 == torch.float16 else RN_BF16, int(self._decoupled),
                                              blk.data_ptr(), scale.data_ptr() if scale is not None else None,
                                              found.data_ptr() if found is not None else None, torch.cuda.current_stream().cuda_stream),
                      "rn_adam_master_step")
        from . import biasact
        biasact.invalidate_dgrad_weights()           # (the kernel wrote the parameters through raw pointers: no version counter moved)
        return loss

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
                 amsgrad: bool = False, *, maximize: bool = False):
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad, maximize=maximize)


class MasterAdamW(_MasterAdamBase):
    "``torch.optim.AdamW`` (decoupled weight decay: w *= 1 - lr * weight_decay) on fp32 masters, capturable: see ``_MasterAdamBase``."
    _decoupled = True

    def __init__(self, params: Iterable, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 amsgrad: bool = False, *, maximize: bool = False):
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad, maximize=maximize)
