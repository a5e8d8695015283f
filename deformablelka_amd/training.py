"""The trainer-side hooks of the 3-D net: what ``d_lka_former_trainer_synapse.py`` does around the network —
``initialize_network`` (:158-198), ``initialize_optimizer_and_scheduler`` (:200-205) and ``run_iteration`` (:259-309) — plus the
data-parallel wrapper the reference leaves to ``nn.DataParallel`` (``run_training.py``): one process per GPU, ``torch.distributed``
(backend ``nccl`` = RCCL over xGMI), gradients averaged with bucketed all-reduces that overlap the backward pass
(``DistributedDataParallel``), batch sharded by rank with no other collective."""
from __future__ import annotations

from typing import Callable, Sequence

import torch
import torch.nn as nn

from . import inference
from .losses import DC_and_CE_loss, MultipleOutputLoss2
from .network import D_LKA_Former
from .transformerblock import TransformerBlock_3D_single_deform_LKA


def initialize_network(input_channels: int = 1, num_classes: int = 14, crop_size: Sequence[int] = (64, 128, 128), depths=(3, 3, 3, 3),
                       skip_connections=(True, True, True, True), trans_block=TransformerBlock_3D_single_deform_LKA, device=None,
                       patch_size=(2, 4, 4), wgrad_overlap: bool = True) -> D_LKA_Former:
    """d_lka_former_trainer_synapse.py:158-185 (the fvcore FLOP count of :186-193 is logging only).
    wgrad_overlap: the D-LKA transformer blocks issue their weight gradients on a side stream joined at the end of ``backward()`` (transformerblock.WgradOverlap: the
    block-stack engine's schedule for the nn.Module path).  Right for this trainer's loop (``run_iteration``: zero_grad(set_to_none) -> backward -> clip -> step);
    ``wrap_data_parallel`` switches it off again, DistributedDataParallel reads gradients while the pass is still running."""
    net = D_LKA_Former(in_channels=input_channels, out_channels=num_classes, img_size=crop_size, feature_size=16, num_heads=4, depths=list(depths),
                       dims=[32, 64, 128, 256], do_ds=True, trans_block=trans_block, skip_connections=list(skip_connections), patch_size=patch_size)
    if device is not None:
        net = net.to(device)
    net.inference_apply_nonlin = inference.softmax_helper   # the HIP tile blend fuses it (inference.predict_3d_tiled)
    set_wgrad_overlap(net, wgrad_overlap)
    return net


def set_wgrad_overlap(net: nn.Module, on: bool) -> int:
    """Switch the side-stream weight-gradient schedule of every D-LKA transformer block of `net` (see transformerblock.WgradOverlap for its contract); returns how many."""
    n = 0
    for m in net.modules():
        if hasattr(type(m), "wgrad_overlap"):
            m.wgrad_overlap = bool(on)
            n += 1
    return n


def initialize_optimizer(net: nn.Module, initial_lr: float = None, weight_decay: float = None, fused=None, *, algorithm: str = "sgd"):
    """:200-205: SGD, momentum 0.99, Nesterov (``initial_lr`` 1e-2, ``weight_decay`` 3e-5); the reference drives the learning rate with nnU-Net's
    poly schedule.
    ``fused`` (default: on when every parameter is a floating-point GPU tensor) selects torch.optim.SGD's single-pass implementation — the same update,
    weight decay, momentum, Nesterov step and parameter write in one kernel per tensor list instead of the four ``_foreach`` passes over the 42 M parameters
    (0.9 ms of a 30 ms iteration).  ``fused="hip"`` returns ``optim.SGD`` instead: the clip and the step on the library's own multi-tensor kernels, the
    learning rate in device memory (``run_iteration`` and ``GraphedIteration`` recognise it).
    ``algorithm`` (with ``fused="hip"`` only) selects the other trainers' rows on the same kernels: ``"adam"``, the 3-D base trainers'
    ``optim.Adam(3e-4, weight_decay=3e-5, amsgrad=True)`` (Trainer_synapse.py:270-273, Trainer_acdc.py:269-272; they run it under
    ``ReduceLROnPlateau``, which writes ``param_groups`` as any torch scheduler does); ``"adamw"``, the 2-D plain-LKA trainer's
    ``optim.AdamW(0.05, weight_decay=1e-4)`` (2D/trainer_MaxViT_LKA.py:114; base_lr: the 2-D train scripts' default).  ``initial_lr`` and
    ``weight_decay`` left at ``None`` take the selected row's values."""
    rows = {"sgd": (1e-2, 3e-5), "adam": (3e-4, 3e-5), "adamw": (0.05, 1e-4)}
    if algorithm not in rows:
        raise ValueError(f"initialize_optimizer: algorithm must be 'sgd', 'adam' or 'adamw', got {algorithm!r}")
    if algorithm != "sgd" and fused != "hip":
        raise ValueError(f"initialize_optimizer: algorithm={algorithm!r} is built on the library's kernels only, pass fused='hip'")
    initial_lr = rows[algorithm][0] if initial_lr is None else initial_lr
    weight_decay = rows[algorithm][1] if weight_decay is None else weight_decay
    params = list(net.parameters())
    if isinstance(fused, str):
        if fused != "hip":
            raise ValueError(f"initialize_optimizer: fused must be None, a bool or 'hip', got {fused!r}")
        from . import optim
        if algorithm == "adam":
            return optim.Adam(params, initial_lr, weight_decay=weight_decay, amsgrad=True)
        if algorithm == "adamw":
            return optim.AdamW(params, initial_lr, weight_decay=weight_decay)
        return optim.SGD(params, initial_lr, momentum=0.99, nesterov=True, weight_decay=weight_decay)
    if fused is None:
        fused = bool(params) and all(p.is_cuda and p.is_floating_point() for p in params)
    kw = dict(weight_decay=weight_decay, momentum=0.99, nesterov=True)
    if fused:
        try:
            return torch.optim.SGD(params, initial_lr, fused=True, **kw)
        except (RuntimeError, TypeError, ValueError):   # a torch build without the fused implementation for this device
            pass
    return torch.optim.SGD(params, initial_lr, **kw)


def wrap_data_parallel(net: nn.Module, device, find_unused_parameters: bool = False, bucket_cap_mb: int = 25) -> nn.Module:
    """One replica per process / GPU.  ``find_unused_parameters`` is needed for the 2-D net only (its ``decoder_3`` owns two D-LKA blocks
    that never run).  ``gradient_as_bucket_view`` lets RCCL reduce in place.  Without an initialised process group (single
    GPU) the network is returned as is."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return net
    dev = torch.device(device)
    ids = [dev.index] if dev.type == "cuda" else None
    set_wgrad_overlap(net, False)   # (DDP's bucket hooks read a gradient as soon as autograd hands it over: it must be complete by then)
    return nn.parallel.DistributedDataParallel(net, device_ids=ids, find_unused_parameters=find_unused_parameters, bucket_cap_mb=bucket_cap_mb,
                                               gradient_as_bucket_view=True)


def deep_supervision_loss(outputs, target, weights=None, base_loss: Callable = None):
    """The trainer weights the deep-supervision heads 1, 1/2, 1/4, ... (normalised; nnU-Net's ``MultipleOutputLoss2``).  ``base_loss``
    defaults to cross-entropy (the reference adds a soft-Dice term from nnU-Net, outside the hot path).  target: the list of label volumes at
    the heads' resolutions, or one full-resolution volume that is nearest-neighbour down-sampled here."""
    base_loss = base_loss or nn.functional.cross_entropy
    if not isinstance(outputs, (list, tuple)):
        return base_loss(outputs, target)
    n = len(outputs)
    weights = weights or [1.0 / (2 ** i) for i in range(n)]
    s = sum(weights)
    total = 0.0
    for i, out in enumerate(outputs):
        tgt = target[i] if isinstance(target, (list, tuple)) else target
        if tgt.shape[-3:] != out.shape[-3:]:
            tgt = nn.functional.interpolate(tgt[:, None].float(), size=out.shape[-3:], mode="nearest")[:, 0].long()
        total = total + (weights[i] / s) * base_loss(out, tgt)
    return total


class DeepSupervisionDiceCE(MultipleOutputLoss2):
    """``MultipleOutputLoss2`` as the 3-D trainer wraps its loss, which also takes ONE full-resolution label volume ((B, 1, *) or (B, *)) in place of the
    list the reference's data loader delivers: it is then nearest-neighbour down-sampled to each head's extents (as ``deep_supervision_loss`` does)."""

    def forward(self, x, y):
        if isinstance(y, torch.Tensor):
            if y.ndim == x[0].ndim - 1:
                y = y[:, None]
            full = y if y.is_floating_point() else y.float()
            y = [y if y.shape[2:] == out.shape[2:] else nn.functional.interpolate(full, size=out.shape[2:], mode="nearest") for out in x]
        return super().forward(x, y)


def initialize_loss(deep_supervision: bool = True, num_heads: int = 3, batch_dice: bool = True):
    """What the 3-D trainer steps: ``DC_and_CE_loss({'batch_dice': batch_dice, 'smooth': 1e-5, 'do_bg': False}, {})`` (Trainer_synapse.py:109) on the fused HIP
    kernels (``losses.py``), wrapped for deep supervision with the weights 1, 1/2, 1/4, ... normalised to sum 1 (d_lka_former_trainer_synapse.py:99-108).
    Pass it as ``loss_fn`` to ``run_iteration`` / ``GraphedIteration``; their default stays ``deep_supervision_loss``."""
    loss = DC_and_CE_loss({"batch_dice": batch_dice, "smooth": 1e-5, "do_bg": False}, {})
    if not deep_supervision:
        return loss
    weights = [1.0 / (2 ** i) for i in range(num_heads)]
    total = sum(weights)
    return DeepSupervisionDiceCE(loss, [w / total for w in weights])


def run_iteration(net: nn.Module, optimizer, data: torch.Tensor, target, loss_fn: Callable = deep_supervision_loss, do_backprop: bool = True,
                  clip_norm: float = 12.0, bf16_autocast: bool = False, forward: Callable = None):
    """:259-309: zero_grad, forward, loss, backward, clip_grad_norm_(12), step.  ``bf16_autocast`` wraps forward + loss in
    ``torch.autocast(dtype=bfloat16)`` (bf16 needs no gradient scaler — the reference's fp16 branch does, :281-290).  What that changes HERE: torch's own
    layers (norms, activations, the loss) follow autocast; each of the 21 ``TransformerBlock_3D_single_deform_LKA`` wrappers runs MIXED — its D-LKA
    attention on bf16 activations (``dlka_tblock3d_*`` with dtype = DLKA_BF16: the token kernels' bf16 path), its own residual stream, LayerNorm /
    BatchNorm statistics and UnetResBlock convs in fp32 — and the conv re-expressions of ``network.Convolution`` stay fp32 GEMMs."""
    fwd = forward if forward is not None else net      # (modules whose forward takes more than the data tensor)
    optimizer.zero_grad()
    if bf16_autocast:
        with torch.autocast(data.device.type, dtype=torch.bfloat16):
            output = fwd(data)
            loss = loss_fn(output, target)
    else:
        output = fwd(data)
        loss = loss_fn(output, target)
    if do_backprop:
        loss.backward()
        if getattr(optimizer, "clips_in_step", False):   # optim.SGD: one norm pass, then the clip factor applied inside the update pass
            optimizer.step(max_grad_norm=clip_norm)
        else:
            torch.nn.utils.clip_grad_norm_(net.parameters(), clip_norm)
            optimizer.step()
    return loss.detach()


class GraphedIteration:
    """``run_iteration`` captured ONCE in a hipGraph and replayed: forward, loss, backward, ``clip_grad_norm_`` and the optimizer step become one
    graph launch per iteration (the D-LKA autograd Functions launch on the capturing stream; every tensor the iteration creates comes from the
    graph's private pool).  Static shapes: ``data`` / ``target`` are copied into the captured input buffers.  The learning rate is read when the graph
    is captured — build a new one after changing it (the reference's poly schedule changes it once per EPOCH); a call with a changed rate raises
    instead of silently stepping with the old one.  With ``optim.SGD`` (``initialize_optimizer(fused="hip")``) the rate lives in device memory and a
    changed value is uploaded in front of the replay instead.  Returns a COPY of the loss (the captured buffer is overwritten by the next replay).  BatchNorm
    layers with ``momentum=None`` are rejected (host read of ``num_batches_tracked``).  Single process; with ``DistributedDataParallel`` use the
    eager ``run_iteration``."""

    def __init__(self, net: nn.Module, optimizer, data: torch.Tensor, target: torch.Tensor, loss_fn: Callable = deep_supervision_loss,
                 clip_norm: float = 12.0, warmup: int = 3):
        if not data.is_cuda:
            raise RuntimeError("GraphedIteration needs GPU tensors")
        for name, m in net.named_modules():   # cumulative-average BatchNorm reads num_batches_tracked on the HOST every step: a device sync inside the
            if isinstance(m, nn.modules.batchnorm._BatchNorm) and m.track_running_stats and m.momentum is None:   # capture, or a value baked into the graph
                raise RuntimeError(f"GraphedIteration: BatchNorm layer {name!r} has momentum=None (cumulative moving average), which cannot be captured "
                                   "in a hipGraph; give it a momentum or use the eager run_iteration")
        self.net, self.optimizer = net, optimizer
        self._captured_lrs = [float(g["lr"]) for g in optimizer.param_groups]   # the graph holds these values (see __call__)
        self.data, self.target = data.clone(), target.clone()
        side = torch.cuda.Stream(device=data.device)
        side.wait_stream(torch.cuda.current_stream(data.device))
        with torch.cuda.stream(side):   # warm-up off the default stream: optimizer state, lazily built tables and workspaces exist before the capture
            for _ in range(max(1, warmup)):
                run_iteration(net, optimizer, self.data, self.target, loss_fn, True, clip_norm)
        torch.cuda.current_stream(data.device).wait_stream(side)
        optimizer.zero_grad(set_to_none=True)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.loss = run_iteration(net, optimizer, self.data, self.target, loss_fn, True, clip_norm)

    def __call__(self, data: torch.Tensor = None, target: torch.Tensor = None) -> torch.Tensor:
        if data is not None:
            self.data.copy_(data, non_blocking=True)
        if target is not None:
            self.target.copy_(target, non_blocking=True)
        lrs = [float(g["lr"]) for g in self.optimizer.param_groups]
        if getattr(self.optimizer, "lr_on_device", False):
            self.optimizer.sync_lr()   # optim.SGD: the captured step reads the rate from device memory; a changed one is uploaded in front of the replay
        elif lrs != self._captured_lrs:
            raise RuntimeError(f"GraphedIteration: the optimizer's learning rate changed ({self._captured_lrs} -> {lrs}) but the captured graph holds the "
                               "old value; build a new GraphedIteration after changing it")
        self.graph.replay()
        return self.loss.clone()   # (a copy: ``self.loss`` is the graph's static output buffer, overwritten by the next replay)


def augmented_batches(loader, augmentation):
    """The trainer's ``tr_gen`` with the transform chain on the device: every batch of ``loader`` (a dict with 'data' (B, C, D, H, W) and 'seg',
    as the reference's DataLoader3D yields them) goes through ``augmentation`` (``augmentation.MoreDAAugmentation``) and comes out as
    ``(data, target)`` for ``run_iteration(net, optimizer, data, target, loss_fn=initialize_loss())``."""
    for batch in loader:
        out = augmentation(batch["data"], batch["seg"])
        yield out["data"], out["target"]
