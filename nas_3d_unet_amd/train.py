"""Train-step / search-step harness: the build's counterpart of the reference's hot loops
(train.py:117-128: zero_grad -> forward -> Dice -> backward -> Adam.step;
 search.py:211-238: architecture step on the validation batch, then weight step on the train batch).

MI355X-first mechanics (none of which the reference has):
  * all kernel weights live in ONE flat fp32 buffer, their gradients in a second one; backward
    kernels write gradients in place (no per-tensor accumulate launches) and ONE fused Adam
    launch updates everything (n3d_adam_step);
  * forward + backward (+ Adam) of a fixed-shape step is captured once into a HIP graph and
    replayed, which removes the per-kernel host launch cost (~300 launches per step);
  * data parallel: one process per GPU, parameters broadcast once, per step a SUM all-reduce of the flat gradient buffer over
    RCCL through the C ABI's n3d_comm_* on ONE communicator per process (comm.py: no torch.distributed collective inside the step,
    so nothing of ProcessGroupNCCL's watchdog can meet a stream capture), the mean folded into the Adam kernel.  Default: ONE
    bucket issued from the step's own stream behind the step's graphs.  n_buckets >= 2: on the side-stream schedule a bucket that
    the backward walk has completed is reduced and all-reduced ON THE WEIGHT-GRADIENT STREAM under the rest of the backward
    (device flags, no host wait); without a side schedule the exchange stays a single bucket.
"""
from __future__ import annotations

import contextlib
import os
import types
import weakref

import torch
import torch.distributed as dist

from . import comm as _comm
from . import fused as _fused
from . import kernels as K
from .loss import BoundaryLoss, TverskyBCELoss, WeightedDiceLoss


def _loss_of(model, loss_fn, x, t):
    """loss of the model on (x, t): through the model's fused head + loss path when it has one"""
    fl = getattr(model, "forward_loss", None)
    if fl is not None and isinstance(loss_fn, WeightedDiceLoss):
        return fl(x, t, loss_fn.smooth)[0]
    if fl is not None and isinstance(loss_fn, (TverskyBCELoss, BoundaryLoss)):
        return fl(x, t, loss=loss_fn)[0]
    return loss_fn(model(x), t)


def _trainer_loss(loss, kernel):
    """the loss a trainer trains `kernel` with: WeightedDiceLoss() by default, or the caller's WeightedDiceLoss / TverskyBCELoss -- whose
    cross-entropy term needs the fused three-channel head (head.check_loss_head raises with the reason) --, or a BoundaryLoss, whose
    boundary term needs that head too"""
    if loss is None:
        return WeightedDiceLoss()
    if not isinstance(loss, (WeightedDiceLoss, TverskyBCELoss, BoundaryLoss)):
        raise TypeError("loss must be a WeightedDiceLoss, a TverskyBCELoss or a BoundaryLoss (got %s)" % type(loss).__name__)
    from . import head as _head
    head = getattr(kernel, "last_conv", None)
    if head is not None:
        _head.check_loss_head(head, loss)
    elif isinstance(loss, BoundaryLoss):
        raise K.N3DError("BoundaryLoss: the boundary term is formed inside the fused head, and this model has no `last_conv` head")
    elif isinstance(loss, TverskyBCELoss) and loss.bce_weight > 0:
        raise K.N3DError("TverskyBCELoss(bce_weight=%g): the cross-entropy term is formed inside the fused head, and this model has no "
                         "`last_conv` head" % loss.bce_weight)
    return loss


GRAD_HEADER = 4   # floats in front of a flat gradient buffer (FlatParams.grad_full)


class FlatParams:
    """Re-homes a list of parameters into one flat buffer (+ a flat gradient buffer)."""

    def __init__(self, params, device):
        self.params = [p for p in params]
        offs, n = [], 0
        for p in self.params:
            offs.append(n)
            n += (p.numel() + 3) // 4 * 4  # keep every tensor 16-byte aligned
        self.numel = n
        self.flat = torch.zeros(n, dtype=torch.float32, device=device)
        # 16 bytes in front of the gradients: word 0 is the "a stream hand-off of this rank timed out" flag that data-parallel
        # ranks SUM-all-reduce together with the gradients (GradSync), so that every rank withholds the same update
        self.grad_full = torch.zeros(n + GRAD_HEADER, dtype=torch.float32, device=device)
        self.grad = self.grad_full[GRAD_HEADER:]
        self.exp_avg = torch.zeros(n, dtype=torch.float32, device=device)
        self.exp_avg_sq = torch.zeros(n, dtype=torch.float32, device=device)
        self.max_exp_avg_sq = None      # (AMSBound only: ensure_amsbound)
        self.step = K.step_counter(device) if torch.device(device).type == "cuda" else torch.zeros(1, dtype=torch.int32, device=device)
        self.offsets = offs
        with torch.no_grad():
            for p, o in zip(self.params, offs):
                v = self.flat[o:o + p.numel()].view(p.shape)
                v.copy_(p.data)
                p.data = v
                g = self.grad[o:o + p.numel()].view(p.shape)
                p._n3d_grad = g  # backward kernels write here (programs.py / kernels.grad_target)
                p.grad = g

    def adam(self, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, grad_scale=1.0, lr_dev=None, guard=None):
        K.adam_step(self.flat, self.grad, self.exp_avg, self.exp_avg_sq, self.step, lr, betas[0], betas[1], eps,
                    weight_decay, grad_scale, True, lr_dev, guard)

    ema = None          # averaged weights (flat fp32) and their n3d_ema_step state: ensure_ema
    ema_state = None

    def ensure_ema(self):
        """the averaged copy of the weights (train.EMA): allocated only for a trainer that asks for it"""
        if self.ema is None:
            self.ema = torch.zeros_like(self.flat)
            self.ema_state = K.ema_state(self.flat.device, int(self.step.item()))

    def ensure_amsbound(self):
        """the AMSBound buffer (adabound.py:79-81, max_exp_avg_sq): allocated only for an optimiser that asks for it"""
        if self.max_exp_avg_sq is None:
            self.max_exp_avg_sq = torch.zeros_like(self.exp_avg_sq)

    def update(self, optim, lr, grad_scale=1.0, lr_dev=None, guard=None, coef=None):
        """one step of `optim` (an OptimSpec) on the flat buffers; coef: 1-element device tensor holding the clip coefficient
        (K.grad_clip_coef), None = no clipping.  Adam without a coefficient is `adam()`, launch for launch."""
        if optim.name == "sgd":       # (the momentum buffer is exp_avg: torch's momentum_buffer)
            return K.sgd_step(self.flat, self.grad, self.exp_avg if optim.momentum != 0 else None, self.step, lr, optim.momentum,
                              optim.dampening, optim.weight_decay, optim.nesterov, grad_scale, True, lr_dev, guard, coef)
        b1, b2 = optim.betas
        if optim.name == "adamw":
            return K.adamw_step(self.flat, self.grad, self.exp_avg, self.exp_avg_sq, self.step, lr, b1, b2, optim.eps, optim.weight_decay,
                                grad_scale, True, lr_dev, guard, coef)
        if optim.name == "adam":
            if coef is None:
                return self.adam(lr, optim.betas, optim.eps, optim.weight_decay, grad_scale, lr_dev, guard)
            return K.adam_step_coef(self.flat, self.grad, self.exp_avg, self.exp_avg_sq, self.step, lr, b1, b2, optim.eps,
                                    optim.weight_decay, grad_scale, True, lr_dev, guard, coef)
        if optim.amsbound:
            self.ensure_amsbound()
        K.adabound_step(self.flat, self.grad, self.exp_avg, self.exp_avg_sq, self.step, lr, b1, b2, optim.eps, optim.weight_decay,
                        grad_scale, True, lr_dev, guard, coef, optim.final_lr, optim.gamma, optim.base_lr,
                        self.max_exp_avg_sq if optim.amsbound else None, optim.name == "adaboundw")


class OptimSpec:
    """Which optimiser a trainer runs on its kernel weights and with what constants: "adam" (torch.optim.Adam defaults,
    train.py:49), "adabound" or "adaboundw" (the reference's adabound.py, imported by train.py:10 / search.py:14).  optim_args
    are the reference classes' keyword arguments next to lr / betas / eps: final_lr, gamma, weight_decay, amsbound; validation
    as adabound.py:27-38.  base_lr is the rate the run started with, as the fp32 value the device scalar holds (adabound.py:43)."""

    NAMES = ("adam", "adabound", "adaboundw")
    ARGS = dict(final_lr=0.1, gamma=1e-3, weight_decay=0, amsbound=False)

    def __init__(self, name="adam", lr=1e-3, betas=(0.9, 0.999), eps=1e-8, optim_args=None):
        if name not in self.NAMES:
            raise ValueError("Invalid optimizer: %r (one of %s)" % (name, ", ".join(self.NAMES)))
        args = dict(optim_args or {})
        unknown = sorted(set(args) - set(self.ARGS))
        if unknown or (name == "adam" and args):
            raise ValueError("Invalid optim_args for %s: %s" % (name, unknown or sorted(args)))
        args = {**self.ARGS, **args}
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: {}".format(lr))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: {}".format(eps))
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError("Invalid beta parameter at index 0: {}".format(betas[0]))
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameter at index 1: {}".format(betas[1]))
        if not 0.0 <= args["final_lr"]:
            raise ValueError("Invalid final learning rate: {}".format(args["final_lr"]))
        if not 0.0 <= args["gamma"] < 1.0:
            raise ValueError("Invalid gamma parameter: {}".format(args["gamma"]))
        if name != "adam" and not 0.0 < lr:
            raise ValueError("Invalid learning rate: {} (the bounds scale with lr / base_lr)".format(lr))
        self.name, self.betas, self.eps = name, (float(betas[0]), float(betas[1])), float(eps)
        self.final_lr, self.gamma = float(args["final_lr"]), float(args["gamma"])
        self.weight_decay, self.amsbound = float(args["weight_decay"]), bool(args["amsbound"])
        self.base_lr = float(torch.tensor(float(lr), dtype=torch.float32))


class SGD:
    """`optimizer=SGD(momentum=0.99, nesterov=True, weight_decay=3e-5)`: torch.optim.SGD (maximize=False) on the flat buffers, one
    guarded launch (n3d_sgd_step).  Validation as torch's class; the learning rate is the trainer's `lr`."""

    name = "sgd"
    amsbound = False

    def __init__(self, momentum=0.0, nesterov=False, dampening=0.0, weight_decay=0.0):
        if momentum < 0.0:
            raise ValueError("Invalid momentum value: {}".format(momentum))
        if weight_decay < 0.0:
            raise ValueError("Invalid weight_decay value: {}".format(weight_decay))
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        self.momentum, self.dampening, self.weight_decay, self.nesterov = float(momentum), float(dampening), float(weight_decay), bool(nesterov)

    def bound(self, lr):
        if lr < 0.0:
            raise ValueError("Invalid learning rate: {}".format(lr))
        return self


class AdamW:
    """`optimizer=AdamW(betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)`: torch.optim.AdamW (amsgrad=False) on the flat buffers,
    one guarded launch (n3d_adamw_step).  Validation as torch's class; the learning rate is the trainer's `lr`."""

    name = "adamw"
    amsbound = False

    def __init__(self, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: {}".format(eps))
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError("Invalid beta parameter at index 0: {}".format(betas[0]))
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameter at index 1: {}".format(betas[1]))
        if not 0.0 <= weight_decay:
            raise ValueError("Invalid weight_decay value: {}".format(weight_decay))
        self.betas, self.eps, self.weight_decay = (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)

    bound = SGD.bound


def _optim_spec(optimizer, lr, betas, eps, optim_args):
    """a trainer's optimiser: one of OptimSpec's three names with optim_args, or an SGD / AdamW spec object (which carries its
    own constants: optim_args do not apply)"""
    if isinstance(optimizer, (SGD, AdamW)):
        if optim_args:
            raise ValueError("optim_args do not apply to optimizer=%s(...): pass them to the spec object" % type(optimizer).__name__)
        return optimizer.bound(lr)
    return OptimSpec(optimizer, lr, betas, eps, optim_args)


class _LRSchedule:
    """A per-update learning-rate rule evaluated ON THE DEVICE from the device step counter, inside the captured step
    (n3d_lr_schedule): linear warm-up from warmup_start * lr to lr over warmup_steps updates, then the subclass's decay until
    total_steps, then its end value.  The closed form of torch's SequentialLR([LinearLR, PolynomialLR | CosineAnnealingLR])."""

    kind = None
    FIELDS = ("total_steps", "power", "warmup_steps", "warmup_start", "min_lr")

    def __init__(self, total_steps, power=1.0, warmup_steps=0, warmup_start=0.1, min_lr=0.0):
        if int(total_steps) != total_steps or int(warmup_steps) != warmup_steps or not 0 <= warmup_steps < total_steps:
            raise ValueError("schedule: total_steps and warmup_steps are integers with 0 <= warmup_steps < total_steps (got %r, %r)"
                             % (total_steps, warmup_steps))
        if not 0.0 <= warmup_start <= 1.0:
            raise ValueError("schedule: warmup_start is a factor in [0, 1] (got %r)" % (warmup_start,))
        if min_lr < 0.0 or power <= 0.0:
            raise ValueError("schedule: min_lr >= 0 and power > 0 (got %r, %r)" % (min_lr, power))
        self.total_steps, self.warmup_steps = int(total_steps), int(warmup_steps)
        self.power, self.warmup_start, self.min_lr = float(power), float(warmup_start), float(min_lr)

    def state_dict(self):
        return dict(kind=self.name, **{k: getattr(self, k) for k in self.FIELDS})

    def record(self, base_lr, device):
        return K.lr_schedule_record(self.kind, base_lr, self.min_lr, self.warmup_steps, self.warmup_start, self.total_steps, self.power, device)


class PolyLR(_LRSchedule):
    """`schedule=PolyLR(total_steps=T, power=0.9)`: lr * (1 - u / n)^power floored at min_lr (nnU-Net's rule with no warm-up)"""
    name, kind = "poly", K.LR_POLY

    def __init__(self, total_steps, power=0.9, warmup_steps=0, warmup_start=0.1, min_lr=0.0):
        super().__init__(total_steps, power, warmup_steps, warmup_start, min_lr)


class CosineLR(_LRSchedule):
    """`schedule=CosineLR(total_steps=T, warmup_steps=W)`: min_lr + (lr - min_lr) (1 + cos(pi u / n)) / 2"""
    name, kind = "cosine", K.LR_COSINE

    def __init__(self, total_steps, warmup_steps=0, warmup_start=0.1, min_lr=0.0):
        super().__init__(total_steps, 1.0, warmup_steps, warmup_start, min_lr)


class EMA:
    """`ema=EMA(decay=0.999)`: an exponential moving average of the weights (torch's AveragedModel with get_ema_multi_avg_fn(decay)),
    one launch behind every optimiser launch; Trainer.averaged_weights() evaluates and predicts with it"""

    def __init__(self, decay=0.999):
        if not 0.5 < decay < 1.0:
            raise ValueError("EMA: 0.5 < decay < 1 (got %r)" % (decay,))
        self.decay = float(decay)


class _GradClip:
    """global-norm gradient clipping in front of an update (config.yml:49 grad_clip; train.py:126-127, search.py:236-237):
    one launch writes {norm, coefficient} to `out`, the optimiser launch behind it reads the coefficient -- no host sync"""

    def __init__(self, max_norm, device):
        self.max_norm = float(max_norm)
        self.out = torch.zeros(2, dtype=torch.float32, device=device)
        self.scratch = K.grad_clip_scratch(device) if torch.device(device).type == "cuda" else None

    def launch(self, grad, grad_scale):
        K.grad_clip_coef(grad, self.max_norm, self.scratch, self.out, grad_scale)
        return self.out[1:]


class PlateauLR:
    """Host logic of torch.optim.lr_scheduler.ReduceLROnPlateau as the reference uses it
    (`ReduceLROnPlateau(optim, factor=0.5)`, train.py:50; search.py:105-106; stepped once per epoch with the validation
    loss, train.py:77; search.py:155-156): mode 'min', relative threshold 1e-4, patience 10, cooldown 0, min_lr 0,
    eps 1e-8.  `set_lr(new_lr)` is called when the rate changes; the trainers keep the rate in a device scalar that
    the Adam kernel reads, so a captured HIP graph follows the schedule without re-capture."""

    def __init__(self, get_lr, set_lr, factor=0.5, patience=10, threshold=1e-4, cooldown=0, min_lr=0.0, eps=1e-8):
        if factor >= 1.0:
            raise ValueError("Factor should be < 1.0.")
        self.get_lr, self.set_lr = get_lr, set_lr
        self.factor, self.patience, self.threshold, self.cooldown, self.min_lr, self.eps = factor, patience, threshold, cooldown, min_lr, eps
        self.best = float("inf")
        self.num_bad_epochs = 0
        self.cooldown_counter = 0
        self.last_epoch = 0

    def step(self, metric):
        current = float(metric)
        self.last_epoch += 1
        if current < self.best * (1.0 - self.threshold):
            self.best = current
            self.num_bad_epochs = 0
        else:
            self.num_bad_epochs += 1
        if self.cooldown_counter > 0:
            self.cooldown_counter -= 1
            self.num_bad_epochs = 0
        if self.num_bad_epochs > self.patience:
            old = self.get_lr()
            new = max(old * self.factor, self.min_lr)
            if old - new > self.eps:
                self.set_lr(new)
            self.cooldown_counter = self.cooldown
            self.num_bad_epochs = 0
        return self.get_lr()


def _plateau_for(owner, lr_attr, setter):
    """PlateauLR bound to a trainer through a weak reference: no trainer <-> scheduler cycle, so a dropped trainer (and the
    HIP graphs / private memory pool it owns) is released at once by reference counting, never by a cyclic collection that could
    fire in the middle of another trainer's graph capture"""
    ref = weakref.ref(owner)
    return PlateauLR(lambda: getattr(ref(), lr_attr), lambda v: getattr(ref(), setter)(v))


class GradSync:
    """Bucketed SUM all-reduce of one flat gradient buffer; callers divide by the world size (folded into the Adam kernel).

    xGMI is point-to-point (7 links per GPU) and the whole payload is 2-7 MB (searched net) / 27 MB (supernet), so the
    collective is latency-bound: a few large buckets, never one call per tensor.  `ranges`: the buckets as (begin, end)
    element ranges in ISSUE order (default: n_buckets equal slices).
    backend (default: "rccl" for CUDA tensors on an NCCL group, else "torch"):
      "rccl"  = n3d_comm_allreduce_sum on the process's shared communicator (comm.for_group): stream-ordered on the CURRENT stream,
                no Work object, no event, no thread that polls it later -- nothing that can collide with a stream capture
                (comm.py says what did in round 4);
      "torch" = torch.distributed.all_reduce (gloo on CPU tensors; two gloo processes sharing one GPU).  On an NCCL group the call is
                issued on a comm stream of this object's own that is NEVER captured, tied to the current stream by two event waits:
                ProcessGroupNCCL's watchdog polls the Work's end event until it has retired it, and HIP refuses that poll while the
                stream the event was last recorded on is capturing."""

    def __init__(self, flat_grad, process_group=None, n_buckets=2, ranges=None, backend=None, header=None):
        """header: the full buffer `flat_grad` is a view of (FlatParams.grad_full: GRAD_HEADER floats in front of it) -- those
        words are exchanged together with the bucket that is issued LAST (the one that starts at 0)"""
        self.header = header
        self.g = flat_grad
        self.pg = process_group
        self.world = dist.get_world_size(process_group) if dist.is_initialized() else 1
        n = flat_grad.numel()
        nb = max(1, min(n_buckets, n // 4 if n >= 4 else 1))
        self.edges = [n * i // nb // 4 * 4 for i in range(nb)] + [n]
        self.ranges = list(ranges) if ranges is not None else list(zip(self.edges[:-1], self.edges[1:]))
        self.force = dist.is_initialized() and os.environ.get("N3D_FORCE_DP") == "1"  # see Trainer.dp_path
        self.active = self.world > 1 or self.force
        self._comm = None
        self._torch_stream = None
        want = backend or os.environ.get("N3D_COMM") or "rccl"
        if want not in ("rccl", "torch"):
            raise ValueError("GradSync: backend must be 'rccl' or 'torch', not %r" % (want,))
        if self.active and want == "rccl":
            self._comm = _comm.for_group(self.pg, flat_grad.device)     # None: CPU tensors / not an NCCL group -> torch.distributed
        self.backend = "rccl" if self._comm is not None else "torch"
        if self.active and self.backend == "torch" and flat_grad.is_cuda and _comm._is_nccl(self.pg):
            self._torch_stream = torch.cuda.Stream(device=flat_grad.device)

    def close(self):
        """(the communicator is the process's shared one: comm.close_all() destroys it)"""
        self._comm = None

    def reduce_range(self, i):
        """SUM all-reduce of bucket i, ordered on the CURRENT stream"""
        if not self.active:
            return
        a, b = self.ranges[i]
        if b <= a:
            return
        buf = self.g
        if self.header is not None and a == 0 and i == len(self.ranges) - 1:
            buf, b = self.header, b + GRAD_HEADER      # the hand-off flag rides in front of the last bucket
        if self._comm is not None:
            self._comm.allreduce_sum_ptr(buf.data_ptr() + 4 * a, b - a)
        elif self._torch_stream is not None:
            cur, cs = torch.cuda.current_stream(), self._torch_stream
            cs.wait_stream(cur)
            with torch.cuda.stream(cs):
                dist.all_reduce(buf[a:b], op=dist.ReduceOp.SUM, group=self.pg)
            cur.wait_stream(cs)
        else:
            dist.all_reduce(buf[a:b], op=dist.ReduceOp.SUM, group=self.pg)

    def all_reduce(self):
        """sum-reduce every bucket, in issue order"""
        if not self.active:
            return
        for i in range(len(self.ranges)):
            self.reduce_range(i)

    def broadcast(self, t, src=0):
        """rank `src`'s copy of t to every rank (once, when a trainer is built)"""
        if self.world <= 1:
            return
        if self._comm is not None:
            self._comm.broadcast(t, src)
        else:
            dist.broadcast(t, src=dist.get_global_rank(self.pg, src) if self.pg is not None else src, group=self.pg)

    def all_true(self, flag):
        """True only if `flag` is true on every rank (data-parallel ranks must take the same schedule decisions: they decide which
        graphs exist and in which order collectives are issued)"""
        if self.world <= 1:
            return bool(flag)
        if self._comm is not None:
            return self._comm.all_true(flag)
        ok = torch.tensor([1.0 if flag else 0.0], device=self.g.device)
        dist.all_reduce(ok, op=dist.ReduceOp.MIN, group=self.pg)
        return float(ok.item()) != 0.0


_capture_streams = {}


def _dev_key(device):
    """index of a torch device; an index-less 'cuda' means the current device"""
    device = torch.device(device)
    return device.index if device.index is not None else torch.cuda.current_device()


def capture_stream(device):
    """the ONE stream every trainer of this process warms up and captures on.  Streams are hardware queues: with more of them than
    the scheduler keeps resident side by side (four, counting the default stream, on this stack) a device-side wait of the side
    schedule is only relieved at the end of a time slice -- so nothing here makes a stream it does not need"""
    key = _dev_key(device)
    st = _capture_streams.get(key)
    if st is None:
        st = _capture_streams[key] = torch.cuda.Stream(device=device)
    return st


_side_streams = {}   # device index -> [side streams made so far]: trainers share them (every new HIP stream may become another
                     # hardware queue, and with more queues than the scheduler keeps resident a spinning wait kernel is only
                     # relieved at the end of a ~1 ms time slice)


def _low_priority_stream(device):
    """a stream of the LOWEST priority the runtime offers (the side work must not take compute units from the backward chain);
    torch only exposes normal / high, so the stream is made through HIP and wrapped"""
    try:
        with torch.cuda.device(device):
            # (A CU mask on the side stream does not help: hipExtStreamCreateWithCUMask makes a BLOCKING stream -- next to torch's
            # legacy default stream every hand-off then takes a time slice, a 9.6 ms step -- and with the whole step moved to a
            # non-blocking stream, a side stream held to 28 or 24 compute units of every XCD [mask bit i = CU i // 8 of XCD i % 8;
            # a mask that empties an XCD is ignored] leaves the chain's time under the side work where it was, 2.01 ms: what the side
            # work costs the chain is not compute units.  profiles/r03_contention_probes.log)
            h = K.stream_create_low_priority()     # through libn3d: the HIP runtime that launches the kernels makes the stream
        return torch.cuda.ExternalStream(h, device=device)
    except K.N3DError:
        return torch.cuda.Stream(device=device)


def reserve_side_streams(device, n=2):
    """Make the process's side streams NOW and put a launch on each.  Which hardware queue / pipe a HIP stream gets is settled when
    it is first used, in creation order; streams made early sit next to the default stream's queue and run side by side with it,
    while streams made after a lot of other activity were seen to share a time slice with it (a search step of 58 instead of
    14.5 ms; docs/history/DESIGN_r01-r03.md).  Every trainer calls this first; a program that does other GPU work before it builds a
    trainer can call it right after selecting the device.  (A late reservation is not an error: the trainers time both schedules
    and keep the single-stream one if the side streams do not pay.)"""
    device = torch.device(device)
    if device.type != "cuda":
        return []
    pool = _side_streams.setdefault(_dev_key(device), [])
    made = False
    while len(pool) < n:
        pool.append(_low_priority_stream(device))
        made = True
    if made:
        scratch = torch.zeros(8, dtype=torch.int32, device=device)
        scratch[0] = 1
        for st in pool:
            with K.on_side(st):
                K.sync_signal(scratch.data_ptr() + 16, scratch.data_ptr(), False)
        torch.cuda.synchronize(device)
    return pool


class SideSchedule:
    """Weight-gradient kernels on a SIDE HIP stream, tied to the backward chain by flags in device memory (include/n3d.h,
    "stream hand-off"; round 3).

    Nothing on the backward chain waits for a weight gradient until the slab reduction in front of Adam, and the chain is
    latency-bound (a few workgroups per launch), so the chip has room for them next to it.  With `deferring()` active the
    weight-gradient launches are queued (kernels.StepContext.wq); at a cut point -- the end of a node / cell of the backward
    walk with at least `min_queue` launches queued, and the end of the walk -- the main stream stores the step number to a
    flag and the queue gets a mark.  `launch_side()` (on the side stream) then issues, per mark, a one-lane wait kernel on
    that flag followed by the queued kernels, and publishes a 'done' flag; `finish()` (main stream) waits for it and runs the
    slab reduction.  Main chain, side work and tail are replayed as three separately launched HIP graphs: an event between
    graph launches costs ~190 us per hand-off on this stack and an intra-graph fork ~19 us per edge without overlapping, a
    flag costs a ~2 us kernel on each side (profiles/r03_handoff_cost.log).
    Device words of `sync` (int32): [0] main-stream step, [1] time-outs, [2] side-stream step, [3] weight-gradient stream step,
    [4] time-outs the host has acknowledged, [8 + i] flag of cut i, [8 + JOIN] side work of this step done.

    A wait that gives up lets its stream go on (never a hung GPU), so the step's gradients may be wrong.  That must not reach the
    weights: every optimizer launch of a trainer with a SideSchedule is GUARDED (`guard()`, n3d_adam_step_guarded) -- while
    sync[1] != sync[4] it updates nothing, writes NaN to the loss and sets a host-visible word.  The trainers poll that word at
    every step() (no HIP call) and at every host-visible point (check()); a time-out is FATAL for the schedule: the trainer
    raises until `acknowledge()` (Trainer.recover) has been called, which also retires the side schedule."""
    JOIN = 400

    def __init__(self, device, ctx, min_queue=None, wgrad_stream=False, tail_inline=(2,), early_finalize=0):
        """wgrad_stream: a SECOND side stream for the weight-gradient launches (the supernet's weight pass keeps the first one busy
        with the preprocess-fed edges of its forward and backward); without it, or when no second stream passes the probe, the
        weight gradients share the one side stream.  tail_inline, early_finalize: see below"""
        self.device, self.ctx = device, ctx
        self.min_queue = 5 if min_queue is None else int(min_queue)
        # cuts from the end at which the side stream reduces the slabs it has so far (0 = off, the default: measured at 64^3 the
        # tail shrinks 66 -> 49 us but the reduction takes 24 us out of the chain it runs beside)
        self.early_finalize = early_finalize
        # live cuts: the slabs launched so far are reduced on the weight-gradient stream behind the n-th group (0 = never, -1 = at 55 %
        # of the groups the fullest pass so far had).  64^3 train step: tail 0.078 -> 0.064 ms, chain +0.001 (n = 11 of 20)
        self.early_at = -1
        # weight-gradient groups, counted from the end of the walk, that go to the INLINE side stream instead (see cut()).  (Every k-th
        # group there, or a second weight-gradient stream, measured slower: profiles/r04_alternate_ab.log)
        self.tail_inline = tail_inline
        self._live_cuts = 0
        self._live_cuts_max = 0
        self.sync = torch.zeros(8 + self.JOIN + 8, dtype=torch.int32, device=device)
        self.sync[0] = 1
        self.sync[2] = 1
        self.host_word = K.HostWord()     # set by a guarded update that was withheld
        self.failed = 0                   # time-outs seen and not yet acknowledged (the trainers refuse to step while > 0)
        self._cuts = 0
        self._main_jobs = {}
        self._last_cut = -1
        self._pass_active = False
        self.live = False      # backward_mode(): cuts hand their group to the side stream at once
        self.bwd_side_inputs = (0, 1)   # backward_mode(): the side stream takes the edges fed by these preprocess outputs
        self.arena = []        # every tensor made while forward_mode() / arena_mode() is on: held until finish()
        self.seen = 0
        # N3D_SIDE_TRACE=1 (tools/side_timeline.py): wall-clock stamps next to every hand-off.  int64 words: [0] main: first cut,
        # [2 i + 2] main stored flag i, [2 i + 3] side passed wait i, [2 JOIN + 4] side done, [2 JOIN + 5] main passed the join,
        # [2 JOIN + 6] slab reduction launched behind it, [2 JOIN + 8 + i] the weight-gradient group behind cut i has been launched through
        # (its last kernel is done when the stamp executes: group busy time = this minus [2 i + 3])
        self.trace = torch.zeros(3 * self.JOIN + 16, dtype=torch.int64, device=device) if os.environ.get("N3D_SIDE_TRACE") == "1" else None
        self.stream = self._probe()
        self.wstream = self.stream
        if wgrad_stream and self.stream is not None:
            w = self._probe(exclude=(self.stream,))
            if w is not None:
                self.wstream = w
        self.sync[3] = 1          # the weight-gradient stream's own step counter (used when it is a stream of its own)
        self._side_tok = None     # the side stream's latest flag of this pass (live cuts make the weight-gradient stream wait for it)

    @property
    def split(self):
        return self.wstream is not self.stream

    def wptr(self):
        """step word of the stream that runs the weight gradients"""
        return self.ptr(3) if self.split else self.ptr(2)

    def ptr(self, i):
        return self.sync.data_ptr() + 4 * i

    def _probe(self, exclude=()):
        """a side stream that really runs next to the current one: a few device-side ping-pongs must complete without a time-out
        and fast (a wait kernel at the head of the hardware queue that also carries its signal only ends by its time-out; streams
        that share a time-sliced queue hand over in ~1 ms instead of ~5 us).  Tries a few streams; None = schedule off."""
        import time
        main = torch.cuda.current_stream(self.device)
        rounds = 8
        pool = _side_streams.setdefault(_dev_key(self.device), [])
        for attempt in range(5):
            if attempt < len(pool):
                side = pool[attempt]         # a stream an earlier trainer of this process made: reuse before making another
            else:
                side = _low_priority_stream(self.device) if attempt < 3 else torch.cuda.Stream(device=self.device)
                pool.append(side)
            if any(side is e for e in exclude):
                continue
            ok = True
            for timed in (False, True):      # the first pass also loads the two kernels
                probe = torch.zeros(4 + 2 * rounds, dtype=torch.int32, device=self.device)   # [0] step = 1, [1] time-outs, [4 + i] flags
                probe[0] = 1
                base = probe.data_ptr()
                torch.cuda.synchronize(self.device)
                t0 = time.perf_counter()
                with torch.cuda.stream(side):
                    for i in range(rounds):     # side waits for main's flag i, then publishes its own
                        K.sync_wait(base + 4 * (4 + 2 * i), base, base + 4, False, 20000)   # <= ~10 ms each
                        K.sync_signal(base + 4 * (5 + 2 * i), base, False)
                with torch.cuda.stream(main):
                    for i in range(rounds):
                        K.sync_signal(base + 4 * (4 + 2 * i), base, False)
                        K.sync_wait(base + 4 * (5 + 2 * i), base, base + 4, False, 20000)
                torch.cuda.synchronize(self.device)
                dt = time.perf_counter() - t0
                ok = ok and int(probe[1].item()) == 0 and (not timed or dt < 5e-3)
            if ok:
                return side
        return None

    def guard(self, loss=None, peer_flag=None):
        """UpdateGuard for an optimizer launch behind this schedule's hand-offs (loss: the scalar that turns NaN)"""
        return K.UpdateGuard(self.ptr(1), self.ptr(4), peer_flag, loss.data_ptr() if loss is not None else None, self.host_word.ptr)

    def _fail(self, n):
        raise K.N3DError("side-stream schedule: %d device-side wait(s) timed out -- the streams did not run concurrently.  The updates of "
                         "the affected steps were WITHHELD on the device (weights, Adam moments and step counters are those of the last "
                         "good step; the loss of a withheld step reads NaN).  The trainer refuses to step until recover() is called, "
                         "which acknowledges the time-outs and continues on one stream (N3D_SIDE_WGRAD=0 turns the schedule off)" % n)

    def poll(self):
        """host-only test (no HIP call, no synchronisation): raises if a guarded update has been withheld, or if an earlier
        check() found time-outs that nobody has acknowledged"""
        if self.failed or self.host_word.value:
            if not self.failed:
                self.failed = max(1, int(self.sync[1].item()) - self.seen)
            self._fail(self.failed)

    def check(self):
        """synchronising test: raises if a device-side wait has timed out since the last acknowledge()"""
        n = int(self.sync[1].item())
        if n != self.seen:
            self.failed = n - self.seen
        if self.failed or self.host_word.value:
            self._fail(max(self.failed, 1))

    def sync_timeouts_now(self):
        """the device's time-out counter (synchronises)"""
        return int(self.sync[1].item())

    def acknowledge(self):
        """the caller has dealt with the time-outs (Trainer.recover): updates are allowed again"""
        torch.cuda.synchronize(self.device)
        self.sync[4] = self.sync[1]
        self.seen = int(self.sync[1].item())
        self.failed = 0
        self.host_word.clear()
        torch.cuda.synchronize(self.device)

    class _Deferring:
        def __init__(self, owner):
            self.o = owner

        def __enter__(self):
            o = self.o
            if not o._pass_active:
                o.begin_pass()
            o.ctx.defer_wgrad = True
            self.prev = (_fused.CELL_DONE_HOOK, _fused.NODE_DONE_HOOK)
            outer = self.prev[0]

            def cell(k):
                o.cut(final=k < 0)
                if outer is not None:
                    outer(k)
            _fused.CELL_DONE_HOOK, _fused.NODE_DONE_HOOK = cell, o.cut
            return o

        def __exit__(self, *exc):
            if exc[0] is None:
                self.o.cut(final=True)     # whatever was queued after the last cut of the walk (still on the main stream)
            self.o.ctx.defer_wgrad = False
            _fused.CELL_DONE_HOOK, _fused.NODE_DONE_HOOK = self.prev
            return False

    # -- one pass (forward + backward of one batch) = one step of the flag protocol ------------------------------------------
    def begin_pass(self):
        """flag ids are handed out from 0 within a pass (forward hand-offs and the cuts of the backward walk share them)"""
        self._cuts = 0
        self._live_cuts = 0
        self._main_jobs = {}
        self._last_cut = -1
        self._side_tok = None
        self._pass_active = True

    def _flag(self):
        i = self._cuts
        if i >= self.JOIN:
            raise K.N3DError("side-stream schedule: more than %d hand-offs in one pass" % self.JOIN)
        self._cuts += 1
        return i

    # -- inline side work of the forward pass (fused._run_forward_side) -------------------------------------------------------
    def fork(self):
        """main stream: store a flag behind everything launched so far; returns its id"""
        i = self._flag()
        K.sync_signal(self.ptr(8 + i), self.ptr(0), False, entry=True)     # (under capture: stored by the chain's next kernel as it starts)
        return i

    class _Side:
        def __init__(self, owner, wait_id):
            self.o, self.wait_id = owner, wait_id

        def __enter__(self):
            self.redirect = K.on_side(self.o.stream)
            self.redirect.__enter__()
            K.sync_wait(self.o.ptr(8 + self.wait_id), self.o.ptr(2), self.o.ptr(1), False)
            return self

        def __exit__(self, *exc):
            return self.redirect.__exit__(*exc)

    def side(self, wait_id):
        """with side(flag id): launches go to the side stream, behind a device-side wait on that flag of the main stream"""
        return SideSchedule._Side(self, wait_id)

    def side_signal(self):
        """inside side(): store a flag behind the side stream's launches so far; returns its id"""
        i = self._flag()
        K.sync_signal(self.ptr(8 + i), self.ptr(2), False, entry=True)     # (usually rides in the wait kernel of the next side segment)
        if self.trace is not None:
            K.stamp(self.trace.data_ptr() + 8 * (2 * i + 2))      # (a join flag: the side stream stored it ...)
        self._side_tok = i
        return i

    def join(self, i):
        """main stream: wait for a flag of the side stream"""
        if self.trace is not None:
            K.stamp(self.trace.data_ptr() + 8 * (2 * self.JOIN + 8 + i))   # (... the main stream arrived at its wait ...)
        K.sync_wait(self.ptr(8 + i), self.ptr(0), self.ptr(1), False)
        if self.trace is not None:
            K.stamp(self.trace.data_ptr() + 8 * (2 * i + 3))      # (... and got past it)

    def join_many(self, ids):
        """main stream: wait for several flags of the side stream -- two per launch (n3d_sync_wait2)"""
        ids = list(ids)
        k = 0
        while k + 1 < len(ids):
            a, b = ids[k], ids[k + 1]
            if self.trace is not None:
                for i in (a, b):
                    K.stamp(self.trace.data_ptr() + 8 * (2 * self.JOIN + 8 + i))
            K.sync_wait2(self.ptr(8 + a), self.ptr(8 + b), self.ptr(0), self.ptr(1), False)
            if self.trace is not None:
                for i in (a, b):
                    K.stamp(self.trace.data_ptr() + 8 * (2 * i + 3))
            k += 2
        if k < len(ids):
            self.join(ids[k])

    class _ArenaMode:
        """every tensor created inside (on the calling thread) is held in owner.arena until finish()"""

        def __init__(self, owner):
            self.o = owner

        def __enter__(self):
            from torch.utils._python_dispatch import TorchDispatchMode
            keep = self.o.arena

            class Arena(TorchDispatchMode):
                def __torch_dispatch__(self, func, types, args=(), kwargs=None):
                    out = func(*args, **(kwargs or {}))
                    if isinstance(out, torch.Tensor):
                        keep.append(out)
                    elif isinstance(out, (tuple, list)):
                        keep.extend(t for t in out if isinstance(t, torch.Tensor))
                    return out

            self.mode = Arena()
            self.mode.__enter__()
            return self

        def __exit__(self, *exc):
            return self.mode.__exit__(*exc)

    def arena_mode(self):
        return SideSchedule._ArenaMode(self)

    class _Backward:
        """backward_mode(): supernet cells run the backward of their preprocess-fed edges on the side stream (fused.SIDE_BWD), and
        the schedule is LIVE: a cut of the backward walk hands the weight-gradient launches queued so far to the side stream at
        once (behind a wait on the cut's flag) instead of at the end of the pass -- the side stream is busy during the walk now,
        what is appended at the end would run after all of it"""

        def __init__(self, owner):
            self.o = owner

        def __enter__(self):
            if not self.o._pass_active:
                self.o.begin_pass()
            self.prev, _fused.SIDE_BWD = _fused.SIDE_BWD, self.o
            self.o.live = True
            return self.o

        def __exit__(self, *exc):
            _fused.SIDE_BWD = self.prev
            self.o.live = False
            return False

    def backward_mode(self, side_inputs=(0, 1)):
        self.bwd_side_inputs = tuple(side_inputs)
        return SideSchedule._Backward(self)

    class _Forward:
        """forward_mode(): supernet cells run their off-chain edges on the side stream (fused.SIDE_FWD), and every tensor created
        meanwhile is held in `arena` until finish().  Allocations stay on torch's current stream; with two streams in flight the
        allocator's stream-ordered reuse of a block freed by Python is not ordered against the OTHER stream's pending kernels, so
        nothing made during the pass is released before the streams have joined (a TorchDispatchMode sees every new tensor)."""

        def __init__(self, owner):
            self.o = owner

        def __enter__(self):
            from torch.utils._python_dispatch import TorchDispatchMode
            keep = self.o.arena

            class Arena(TorchDispatchMode):
                def __torch_dispatch__(self, func, types, args=(), kwargs=None):
                    out = func(*args, **(kwargs or {}))
                    if isinstance(out, torch.Tensor):
                        keep.append(out)
                    elif isinstance(out, (tuple, list)):
                        keep.extend(t for t in out if isinstance(t, torch.Tensor))
                    return out

            if not self.o._pass_active:
                self.o.begin_pass()
            self.mode = Arena()
            self.mode.__enter__()
            self.prev, _fused.SIDE_FWD = _fused.SIDE_FWD, self.o
            return self.o

        def __exit__(self, *exc):
            _fused.SIDE_FWD = self.prev
            return self.mode.__exit__(*exc)

    def forward_mode(self):
        return SideSchedule._Forward(self)

    # -- the side stream's work as a HIP graph captured next to torch's capture of the main stream --------------------------------
    def close_bucket(self, on_closed):
        """data parallel, bucketed exchange on device flags: every gradient of a bucket has been LAUNCHED (the backward walk is past
        the cell that completes it).  The weight-gradient stream takes whatever is still queued, waits for the main stream's flag
        behind everything launched so far (and the side stream's latest flag), reduces every slab launched so far -- and
        `on_closed()` then puts the bucket's all-reduce on that stream (eagerly, or as the boundary between two captured segments
        of the stream).  The chain does not wait for anything here."""
        self.cut(final=True)
        i = self.fork()
        with K.on_side(self.wstream):
            word = self.wptr()
            K.sync_wait(self.ptr(8 + i), word, self.ptr(1), False)
            if self.split and self._side_tok is not None:
                K.sync_wait(self.ptr(8 + self._side_tok), word, self.ptr(1), False)
            with K.step_context(self.ctx):
                self.ctx.finalize_now(len(self.ctx.final))
        on_closed()

    def split_wstream_capture(self):
        """end the capture segment of the weight-gradient stream and open the next one (the all-reduce of a closed bucket is
        launched between the two at replay)"""
        st = self.wstream
        self._wsegs.append(K.stream_capture_end(st.cuda_stream))
        K.stream_capture_begin(st.cuda_stream)

    def raw_capture_begin(self):
        """the side stream starts capturing (thread-local mode, like torch's capture of the main stream); launches redirected to it
        while the main stream is being captured land in a graph of their own.  Capture, instantiation and launch go through
        libn3d (n3d_stream_capture_* / n3d_graph_*): the HIP runtime that launches the kernels owns the graphs."""
        self._wsegs = []
        for st in ([self.stream, self.wstream] if self.split else [self.stream]):
            K.stream_capture_begin(st.cuda_stream)

    def raw_capture_end(self):
        """-> [(executable graph handle, stream)] (replayed with raw_replay, released with raw_destroy).  The weight-gradient stream
        may have been captured in several segments (split_wstream_capture): its entries then come in segment order, and
        `self.wseg_count` says how many of the returned entries (the last ones) they are."""
        out, err = [], None
        segs, self._wsegs = self._wsegs, []
        for st in ([self.stream, self.wstream] if self.split else [self.stream]):
            try:
                ex = K.stream_capture_end(st.cuda_stream)
                if st is self.wstream:
                    out.extend((e, st) for e in segs + [ex])
                else:
                    out.append((ex, st))
            except K.N3DError as e:      # end the other stream's capture too before raising
                err = e
        self.wseg_count = len(segs) + 1
        if err is not None:
            self.raw_destroy(out)
            raise err
        return out

    def raw_replay(self, execs):
        for ex, st in execs:
            K.graph_launch(ex, st.cuda_stream)

    @staticmethod
    def raw_destroy(execs):
        for ex, _ in execs or ():
            K.graph_destroy(ex)

    def deferring(self):
        """with side.deferring(): run forward + backward; weight-gradient launches are queued, flags stored at the cut points"""
        return SideSchedule._Deferring(self)

    def cut(self, final=False):
        """a cut point of the backward walk; final (or force) = cut whatever is queued, however little"""
        ctx = self.ctx
        n = ctx.queued()
        if n > 0 and (final or (n >= self.min_queue and self._cuts < self.JOIN - 1)):
            i = self._flag()
            K.sync_signal(self.ptr(8 + i), self.ptr(0), False, entry=True)
            self._main_jobs[i] = len(ctx.final)     # slab-reduction jobs the main chain has issued in front of this flag
            if self.trace is not None:
                K.stamp(self.trace.data_ptr() + 8 * (2 * i + 2))
            if self.live:
                # the side stream takes the group now: wait for the flag, then the launches (their slab-reduction jobs are recorded)
                # the weight-gradient stream is backlogged at the end of the walk (the 64^3-level kernels: the join waited ~45 us
                # behind the chain's last cut, tools/side_timeline.py) while the inline side stream is mostly idle there: the group
                # tail_inline positions from the end (default: the second to last) goes to that stream instead; 1.865 -> 1.85 ms
                inline = self.split and self._live_cuts_max >= 8 and (self._live_cuts_max - self._live_cuts) in self.tail_inline
                with K.on_side(self.stream if inline else self.wstream):
                    word = self.ptr(2) if inline else self.wptr()
                    K.sync_wait(self.ptr(8 + i), word, self.ptr(1), False)
                    if self.split and self._side_tok is not None and not inline:
                        # operands the SIDE stream produced (the d(raw) of its edges): behind its latest flag
                        K.sync_wait(self.ptr(8 + self._side_tok), word, self.ptr(1), False)
                    if self.trace is not None:
                        K.stamp(self.trace.data_ptr() + 8 * (2 * i + 3))
                    ctx.flush_wgrads(inline=inline)
                    if self.trace is not None:
                        K.stamp(self.trace.data_ptr() + 8 * (2 * self.JOIN + 8 + i))
                    self._live_cuts += 1
                    self._live_cuts_max = max(self._live_cuts_max, self._live_cuts)
                    at = self.early_at if self.early_at >= 0 else (int(round(0.55 * self._live_cuts_max)) if self._live_cuts_max >= 8 else 0)
                    if at and self._live_cuts == at and not inline:   # (an inline group runs on the OTHER side stream: the slabs of
                        # the weight-gradient stream's launches are not ordered in front of a reduction issued there)
                        # the slabs of everything launched so far (and of the chain's own jobs in front of this flag) are reduced on
                        # the weight-gradient stream here: the reduction behind the join only has the last groups left
                        ctx.finalize_now(self._main_jobs[i])
                return
            ctx.wq.insert(len(ctx.wq) - n, ("mark", i))    # the wait goes IN FRONT of the launches it guards
            ctx.wq.append(("mark", -1))                    # closes the group (no wait)
            self._last_cut = i

    def launch_side(self, redirect=False):
        """the weight-gradient stream: per group a device-side wait for the main stream's flag, then the queued launches; then the
        'done' flags of this pass (one per side stream).  redirect=False: the caller has made the (single) side stream current;
        True: the launches are redirected here (K.on_side), as the search trainer's simultaneous captures need"""
        marks = [it[1] for it in self.ctx.wq if it[0] == "mark" and it[1] >= 0]
        early = marks[-self.early_finalize] if 0 < self.early_finalize < len(marks) else -1
        prev = {t: (marks[k - 1] if k > 0 else None) for k, t in enumerate(marks)}

        def on_mark(tag):
            if tag >= 0:
                if tag == early and prev[tag] is not None:
                    # the side stream idles between its groups: the slabs of everything it has launched so far (and of the main
                    # chain's own jobs in front of the flag it passed last) are reduced here, so that the reduction behind the join
                    # only has the last few groups left
                    self.ctx.finalize_now(self._main_jobs[prev[tag]])
                K.sync_wait(self.ptr(8 + tag), self.wptr(), self.ptr(1), False)
                if self.trace is not None:
                    K.stamp(self.trace.data_ptr() + 8 * (2 * tag + 3))

        import contextlib
        with (K.on_side(self.wstream) if redirect else contextlib.nullcontext()):
            with K.step_context(self.ctx):
                self.ctx.flush_wgrads(on_mark)
            if self.split:
                K.sync_signal(self.ptr(8 + self.JOIN + 1), self.ptr(3), True)
        with (K.on_side(self.stream) if redirect else contextlib.nullcontext()):
            K.sync_signal(self.ptr(8 + self.JOIN), self.ptr(2), True)
            if self.trace is not None:
                K.stamp(self.trace.data_ptr() + 8 * (2 * self.JOIN + 4))

    def finish(self):
        """on the main stream: wait for the side stream's 'done' flag, then reduce the weight-gradient slabs (one launch)"""
        if self.split:
            K.sync_wait(self.ptr(8 + self.JOIN + 1), self.ptr(0), self.ptr(1), False)
        K.sync_wait(self.ptr(8 + self.JOIN), self.ptr(0), self.ptr(1), True)
        self._pass_active = False
        self.arena.clear()        # (rebinding would orphan the list the dispatch mode of forward_mode() appends to)
        if self.trace is not None:
            K.stamp(self.trace.data_ptr() + 8 * (2 * self.JOIN + 5))
        with K.step_context(self.ctx):
            self.ctx.flush_final()
        if self.trace is not None:
            K.stamp(self.trace.data_ptr() + 8 * (2 * self.JOIN + 6))


class _Ctx:
    """stand-in for an autograd context when a Function's forward / backward are called directly (Trainer's pipeline)"""

    def __init__(self, needs):
        self.needs_input_grad = needs

    def mark_non_differentiable(self, *a):
        pass


def flatten_params(params, device=None):
    """(flat parameter tensor, flat gradient tensor): re-homes every parameter (and its .grad) as a view."""
    params = list(params)
    device = device if device is not None else params[0].device
    offs, n = [], 0
    for p in params:
        offs.append(n)
        n += (p.numel() + 3) // 4 * 4
    flat = torch.zeros(n, dtype=torch.float32, device=device)
    full = torch.zeros(n + GRAD_HEADER, dtype=torch.float32, device=device)   # header: see FlatParams.grad_full
    grad = full[GRAD_HEADER:]
    grad._n3d_full = full
    with torch.no_grad():
        for p, o in zip(params, offs):
            v = flat[o:o + p.numel()].view(p.shape)
            v.copy_(p.data)
            p.data = v
            p.grad = grad[o:o + p.numel()].view(p.shape)
    return flat, grad, offs


def _dropout_states(model):
    return [m._n3d_state for m in model.modules() if getattr(m, "_n3d_state", None) is not None]


def _dropout_snapshot(model, device):
    """snapshot of every Dropout3d generator of the model (created now if a module has not drawn yet)"""
    from . import programs as _P
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout3d):
            _P.dropout_state(m, device)
    return _Snapshot(_dropout_states(model))


class _Snapshot:
    """optimizer-visible state of a trainer (weights, Adam moments, step counters, dropout generators): taken before the
    schedules are timed against each other on the real step, put back afterwards"""

    def __init__(self, tensors):
        self.tensors = [t for t in tensors if t is not None]
        self.saved = [t.clone() for t in self.tensors]

    def restore(self):
        with torch.no_grad():
            for t, v in zip(self.tensors, self.saved):
                t.copy_(v)


def _time_schedule(run, device, warm=2, reps=6):
    import time
    for _ in range(warm):
        run()
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    for _ in range(reps):
        run()
    torch.cuda.synchronize(device)
    return (time.perf_counter() - t0) / reps


class _TwinShell:
    """what SearchTrainer runs for a ShellNet whose kernel net has odd channel counts: the shell's own alphas around the kernel net's
    zero-padded twin (unet.PaddedTwin)"""

    def __init__(self, shell, twin):
        self.shell, self.kernel = shell, twin

    def forward_loss(self, x, t, smooth=1e-6, *, loss=None):
        from . import unet as _unet
        return _unet.run_loss(self.kernel, x, t, tuple(self.shell._soft()), smooth, loss=loss)

    def modules(self):
        return self.kernel.modules()


def _pad_mask_for(tw, real, fp, device):
    """flat 0/1 mask over a FlatParams of a padded twin's parameters: 1 at the real entries"""
    names = {id(q): n for n, q in tw.twin.named_parameters()}
    rshape = {n: q.shape for n, q in real.named_parameters()}
    mask = torch.zeros_like(fp.grad)
    for q, o in zip(fp.params, fp.offsets):
        n = names[id(q)]
        mask[o:o + q.numel()] = tw.embed_tensor(n, torch.ones(rshape[n], device=device), q.shape).reshape(-1)
    return mask


class _GraphTrainer:
    """What Trainer and SearchTrainer share: the zero-padded twin, the side-stream schedule (SideSchedule) and the ranks' agreement
    on it, the guarded gradient exchange, the capture of the plain and the side-stream graphs and the choice between them, the
    captured graphs' input buffers, and what follows a timed-out hand-off.  A subclass supplies its passes: _eager, _warm_up,
    _capture_plain, _side_passes, _replay_plain / _replay_side (which _choose_schedule times) and _replay."""

    N_INPUTS = 2        # tensors step() takes
    TIMING = (2, 6)     # (warm-up, timed) replays of each schedule in _choose_schedule

    def __init__(self, model, kernel, lr, betas, eps, graph, process_group, side_wgrad, loss=None):
        """kernel: the module whose parameters the trainer trains (the model itself, or a shell's kernel net)
        loss: None (WeightedDiceLoss()), a WeightedDiceLoss or a TverskyBCELoss -- a constructor argument, as in the reference, and
        like there no part of a checkpoint"""
        self.model = model
        # channel counts that are not multiples of 4: the trainer trains the kernel module's zero-padded TWIN (unet.PaddedTwin; padded
        # entries have exactly-zero gradients, so Adam never moves them) and cuts the parameters back into it at the host-visible
        # points (check_sync() / sync_to_module()); sync_from_module() re-embeds after its parameters were written from outside
        self._kernel = kernel
        self._twin = None
        if getattr(kernel, "_n3d_padded", False):
            self._twin = kernel._n3d_make_twin()
            self._twin.embed(kernel)
        # side_wgrad (default: N3D_SIDE_WGRAD, on): weight-gradient kernels on side HIP streams (SideSchedule).  Graph mode captures
        # BOTH schedules, times them on the real step and replays the faster one ("force": no comparison)
        env = os.environ.get("N3D_SIDE_WGRAD", "1")
        self.side_wgrad = (env != "0") if side_wgrad is None else bool(side_wgrad)
        self._side_force = side_wgrad == "force" or (side_wgrad is None and env == "force")
        self._side_explicit = side_wgrad is not None     # an eager Trainer (graph=False) takes the side schedule only when asked to
        self.side = None
        self._use_side = False
        self._side_retired = False   # recover() after a timed-out hand-off: the rest of the run stays on one stream
        self.schedule_times = None   # (plain seconds per step, side seconds per step) measured at capture
        self.use_graph = graph
        self._static = None          # the captured graphs' input buffers (input_buffers()); None: the next graph step captures
        self._graph = None           # the plain schedule
        self._side_graphs = None     # the side-stream schedule: per pass (main chain graph, raw side-stream graphs, tail graph)
        self._side_losses = None
        self._side_wsegs = 1         # segments of the last pass' weight-gradient stream graph (Trainer's bucketed exchange cuts it)
        self._n_steps = 0            # step() calls, on every path
        self.pg = process_group
        self.world = dist.get_world_size(process_group) if (process_group is not None or dist.is_initialized()) else 1
        # N3D_FORCE_DP=1: take the multi-GPU code path (all-reduce + eager Adam after the graph) even in a 1-rank group --
        # lets a single-GPU box exercise exactly what N > 1 runs
        self.dp_path = self.world > 1 or (dist.is_initialized() and os.environ.get("N3D_FORCE_DP") == "1")
        self.loss_fn = _trainer_loss(loss, kernel if self._twin is None else self._twin.twin)
        self.lr, self.betas, self.eps = lr, betas, eps
        self.device = next(model.parameters()).device
        if isinstance(self.loss_fn, BoundaryLoss):
            self.loss_fn.weight_tensor(self.device)     # the device scalar exists before any capture reads it
        # evaluation pass (evaluate / eval_result): its accumulator, weight packing, and captured graph with its input buffers
        self._eval_acc = None
        self._eval_ctx = None
        self._eval_static = None
        self._eval_graph = None
        self._eval_loss = None
        reserve_side_streams(self.device)     # first thing on the GPU (see there), also when THIS trainer will not use them

    def _init_side(self, comm, **options):
        """the side-stream schedule (SideSchedule options: wgrad_stream, tail_inline, early_finalize; None without a side stream
        that passes the probe) and the weight-gradient exchange.  Data parallel: the probe is rank-local and timing-based, but every
        rank must take the same schedule decisions (they decide which graphs exist and in which order the collectives go out): the
        side schedule is on only if EVERY rank has one"""
        side = SideSchedule(self.device, self.ctx, **options) if (self.side_wgrad and self.device.type == "cuda") else None
        self.side = side if side is not None and side.stream is not None else None
        self.sync = GradSync(self.fp.grad, self.pg, 1, None, comm, header=self.fp.grad_full)
        if not self.sync.all_true(self.side is not None):
            self.side = None

    def _side_ok(self):
        return self.side is not None and not self._side_retired

    # -- host-visible points ----------------------------------------------------------------------
    def check_sync(self):
        """synchronising check (call it at every host-visible point: before a checkpoint is written, at the end of an epoch, before
        a loss is reported): raises if a device-side wait of the side-stream schedule has timed out.  The updates of such steps
        were withheld on the device, so the weights are those of the last good step; `recover()` continues on one stream."""
        if self.side is not None:
            self.side.check()
        self.sync_to_module()

    def sync_to_module(self):
        """padded twin: the trained parameters back into the user's module (reference shapes); nothing to do otherwise"""
        if self._twin is not None:
            tp = dict(self._twin.twin.named_parameters())
            with torch.no_grad():
                for n, r in self._kernel.named_parameters():
                    r.copy_(self._twin.extract(n, tp[n].detach()))

    def sync_from_module(self):
        """padded twin: the user's module was written from outside (load_state_dict): embed its parameters again"""
        if self._twin is not None:
            self._twin.embed(self._kernel)

    def sync_timeouts(self):
        """device-side waits that have timed out since the trainer was built (synchronises; 0 without a side schedule)"""
        return int(self.side.sync[1].item()) if self.side is not None else 0

    def recover(self):
        """after a time-out (check_sync / step raised): acknowledge it and go on WITHOUT the side-stream schedule.  Nothing has to
        be restored -- the guarded updates of the affected steps never ran -- but those batches are lost to training."""
        if self.side is None:
            return
        self.side.acknowledge()
        self._use_side = False
        self._retire_side_graphs()
        self._side_retired = True
        if self._graph is None:
            self._static = None      # "force" had no plain graph: the next step captures one

    def _retire_side_graphs(self):
        gs, self._side_graphs = self._side_graphs, None
        for g in gs or ():
            SideSchedule.raw_destroy(g[1])

    def close(self):
        """release the raw HIP graphs of the side streams (torch's own graphs and pools go with the object)"""
        try:
            self._retire_side_graphs()
        except Exception:
            pass

    def __del__(self):
        self.close()

    # -- exchange and update guard ----------------------------------------------------------------
    def _exchange(self, sync):
        """data parallel: SUM all-reduce of sync's gradient buffer.  Word 0 of its header: "a hand-off of THIS rank timed out" --
        summed over the ranks with the gradients, so that every rank withholds the same update (a rank without a side schedule
        contributes 0)"""
        if sync.active:
            if self.side is not None:
                K.guard_flag(self.side.ptr(1), self.side.ptr(4), sync.header.data_ptr())
            else:
                sync.header[:1].zero_()
        sync.all_reduce()

    def set_boundary_weight(self, w):
        """move the weight of the trainer's BoundaryLoss: a device scalar the captured step reads, so nothing is recaptured"""
        if not isinstance(self.loss_fn, BoundaryLoss):
            raise K.N3DError("set_boundary_weight: this trainer's loss is a %s, not a BoundaryLoss" % type(self.loss_fn).__name__)
        self.loss_fn.set_weight(w)

    def _prepare_loss(self, t):
        """start of a pass, on the main chain: the signed distance map of the targets for a BoundaryLoss (nothing for another loss)"""
        if isinstance(self.loss_fn, BoundaryLoss):
            from . import head as _head
            _head.prepare_phi(self.loss_fn, t)

    def _guard(self, loss, sync):
        """UpdateGuard of an optimizer launch on sync's gradients (None without a side schedule: nothing can time out)"""
        if self.side is None:
            return None
        return self.side.guard(loss, sync.header.data_ptr() if self.dp_path else None)

    # -- step -------------------------------------------------------------------------------------
    def step(self, *batch):
        """Trainer.step(x, t) -> loss, SearchTrainer.step(x, t, val_x, val_t) -> (architecture-pass loss, weight-pass loss): device
        scalars, no host sync.  With graph=True the first call captures, later calls replay."""
        if self._twin is None:
            return self._step(*batch)
        with _fused.padded_switches():
            return self._step(*batch)

    def _step(self, *batch):
        if self.side is not None:
            self.side.poll()     # host-only: a withheld update (timed-out hand-off) is fatal until recover()
        self._n_steps += 1
        if not self.use_graph:
            return self._eager(*batch)
        self._side_verdict()
        if self._static is None or (self._graph is None and self._side_graphs is None):
            self._capture(batch)
        if not self._copy_in(batch):
            # a batch of another shape (the reference's generator yields a smaller last batch of an epoch) or dtype: the captured
            # graphs are for one only, so this step runs eagerly (same kernels, same update) -- on ONE stream (see Trainer._eager)
            return self._eager(*batch, allow_side=False)
        return self._replay()

    def _copy_in(self, batch):
        """the batch into the captured graphs' input buffers; False (nothing copied) when it does not fit them in shape or dtype.  A
        caller that fills the trainer's own buffers (input_buffers(): the data step writes the batch straight into them) has no
        copy to pay; any other tensor is copied in"""
        for src, dst in zip(batch, self._static):
            if src.shape != dst.shape or src.dtype != dst.dtype:
                return False
        for src, dst in zip(batch, self._static):
            if src is not dst:
                dst.copy_(src)
        return True

    def input_buffers(self):
        """the device buffers the captured graphs read: Trainer (x, t), SearchTrainer (x, t, val_x, val_t); None before the first
        graph step.  A data step that writes a batch straight into them (datastep.patch_batch(out=...)) and passes THESE tensors to
        step() skips the per-step input copy."""
        return self._static if self._static is not None else (None,) * self.N_INPUTS

    def _side_verdict(self):
        """start of a graph step, before anything of it is issued: the replay monitor's verdict (Trainer); nothing here"""

    # -- evaluation -------------------------------------------------------------------------------
    EVAL_THRESHOLD = 0.5     # a voxel is predicted in a region when p >= 0.5 (prediction.py:157-164)

    def evaluate(self, x, t):
        """Evaluation of one validation batch (train.py:138-157 validate(); search.py:251-271): the module the step trains -- its
        padded twin, its storage configuration, the shell's current softmaxed alphas -- in eval mode (no Dropout3d, no generator
        advances), forward only (no autograd graph, no gradient or optimizer state touched), with the Dice loss and the region
        counts of the prediction p >= 0.5 added into the trainer's device accumulator.  Returns the batch loss as a 0-d device
        tensor (no host sync; overwritten by the next replay).  With graph=True the first call captures an evaluation graph of its own
        (one stream, weight packing included, so it reads the weights as they are at replay) and later calls of that shape and dtype
        replay it; another batch shape runs eagerly into the same accumulator.  Not a step: the step count is unchanged."""
        if self._twin is None:
            return self._evaluate(x, t)
        with _fused.padded_switches():
            return self._evaluate(x, t)

    def eval_result(self, reset=True):
        """host-visible point of the evaluation pass (synchronises): the accumulated figures as a head.EvalResult(loss, dice,
        dice_global, n_batches, n_samples); reset=True then zeroes the accumulator in place for the next epoch.  Data parallel:
        COLLECTIVE -- every rank calls it; the accumulators are SUM-all-reduced over the ranks first, so every rank returns the
        figures of all the batches evaluated on any of them."""
        from . import head as _head
        acc = self._eval_accumulator()
        tot = acc
        if self.dp_path:
            tot = acc.clone()
            if self.sync._comm is not None:
                self.sync._comm.allreduce_sum(tot)
            else:
                dist.all_reduce(tot, group=self.pg)
        host = tot.cpu().numpy()
        if reset:
            K.eval_acc_reset(acc)
        return _head.eval_figures(host)

    def eval_accumulator(self):
        """the device accumulator evaluate() adds into (float64, layout of N3D_EVAL_ACC_LEN in include/n3d.h: loss sum, batches, samples,
        then per class hard intersection, predicted and target voxels and the sum of per-sample hard Dice); this rank's only"""
        return self._eval_accumulator()

    def _eval_accumulator(self):
        if self._eval_acc is None:
            self._eval_acc = K.eval_acc(self._kernel.last_conv[0].conv.weight.shape[0], self.device)
        return self._eval_acc

    def _eval_net(self):
        """(the net whose kernels the evaluation runs, its alphas as a callable returning the softmaxed four, or None)"""
        return self.net, None

    def _eval_modules(self):
        seen = {}
        for root in (self.model, self.net):
            for m in root.modules():
                seen.setdefault(id(m), m)
        return list(seen.values())

    def _evaluate(self, x, t):
        self._eval_accumulator()
        if not self.use_graph:
            return self._eval_pass(x, t)
        if self._eval_static is None:
            self._eval_capture(x, t)
        xs, ts = self._eval_static
        if x.shape != xs.shape or x.dtype != xs.dtype or t.shape != ts.shape or t.dtype != ts.dtype:
            return self._eval_pass(x, t)      # (the validation generator's short last batch)
        if x is not xs:
            xs.copy_(x)
        if t is not ts:
            ts.copy_(t)
        self._eval_graph.replay()
        return self._eval_loss

    def _eval_pass(self, x, t):
        """one evaluation pass on the current stream: weight packing, body, evaluation head + accumulation"""
        from . import head as _head, unet as _unet
        if self._eval_ctx is None:
            self._eval_ctx = K.StepContext(self.device)     # the step's packing context stays as the step left it
        net, alphas = self._eval_net()
        mods = self._eval_modules()
        was = [m.training for m in mods]
        try:
            for m in mods:
                m.training = False
            with torch.no_grad(), K.step_context(self._eval_ctx):
                self._eval_ctx.pack_all()
                # (the input layout of the head as unet.run_loss chooses it: node-planar for float targets)
                planar = _unet._head_takes_planar(net) and t.dtype == torch.float32
                body = _unet.body(net, x, alphas() if alphas is not None else None, planar=planar)
                loss = _head.run_eval(net.last_conv, body, t, self._eval_acc, self.loss_fn.smooth, self.EVAL_THRESHOLD, loss=self.loss_fn)
            if not self._eval_ctx.frozen:
                self._eval_ctx.freeze()
        finally:
            for m, w in zip(mods, was):
                m.training = w
        return loss

    def _eval_capture(self, x, t):
        """warm-up passes (allocator, net plan, packing jobs) on the capture stream, then the evaluation graph on one stream; the
        accumulator comes out as it went in"""
        keep = self._eval_acc.clone()
        self._eval_static = (x.clone(), t.clone())
        s = capture_stream(self.device)
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                self._eval_pass(*self._eval_static)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        self._eval_acc.copy_(keep)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            self._eval_loss = self._eval_pass(*self._eval_static)
        self._eval_graph = g

    # -- capture ----------------------------------------------------------------------------------
    def _capture(self, batch):
        """capture (and, with a side stream, choose the schedule); the Dropout3d generators come out as they went in, so the
        masks of the training run do not depend on how many warm-up / timing passes the capture needed"""
        snap = _dropout_snapshot(self.net, self.device)
        try:
            self._static = tuple(a.clone() for a in batch)
            sided = self._side_ok()
            # warm-up on the capture stream (allocator + lazy module state) WITHOUT the optimizer launches: the weights, Adam moments
            # and step counters -- possibly just loaded from a checkpoint (search.py:108-127) -- stay as they are
            s = capture_stream(self.device)
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                for _ in range(2):
                    self._warm_up(sided)
            torch.cuda.current_stream().wait_stream(s)
            torch.cuda.synchronize()
            if sided:
                self._capture_side(s)
                if self._side_force:
                    self._use_side = True
                    return
            self._capture_plain()
            if sided:
                self._choose_schedule()
        finally:
            snap.restore()

    def _capture_side(self, s):
        """The side-stream schedule, per pass (_side_passes: (run the pass' main-stream part, update)) three HIP graphs: the main
        chain (torch capture: forward, Dice, backward with a flag store at every hand-off), the side streams' work behind their
        device-side waits -- captured AT THE SAME TIME as a raw HIP graph, since its launches are issued in the middle of the main
        chain's -- and the tail (wait for the side streams' 'done' flags, slab reduction, Adam unless an exchange sits in between).
        The tail is a graph of its own because the slab-reduction job table is complete only once every weight-gradient launch
        has been issued."""
        import gc
        gc.collect()
        pool = torch.cuda.graph_pool_handle()
        sd = self.side
        torch.cuda.synchronize()
        graphs, losses = [], []
        for run, update in self._side_passes():
            g_main, g_tail = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
            sd.raw_capture_begin()
            try:
                with torch.cuda.stream(s):
                    g_main.capture_begin(pool=pool, capture_error_mode="thread_local")
                    K.entry_capture_begin(s.cuda_stream)      # hand-off signals ride in the entry of the chain's next kernel
                    try:
                        losses.append(run())
                    except BaseException:
                        K.entry_capture_abort(s.cuda_stream)  # (nothing is launched into a capture that has failed)
                        raise
                    K.entry_capture_end(s.cuda_stream)        # ... and what found none goes out before the graph is closed
                    g_main.capture_end()
                sd.launch_side(redirect=True)
            finally:
                side_exec = sd.raw_capture_end()
            with torch.cuda.stream(s):
                g_tail.capture_begin(pool=pool, capture_error_mode="thread_local")
                sd.finish()
                if not self.dp_path:
                    update(losses[-1])
                g_tail.capture_end()
            graphs.append((g_main, side_exec, g_tail))
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        self._side_graphs, self._side_losses, self._side_wsegs = graphs, tuple(losses), sd.wseg_count

    def _state(self):
        """optimizer-visible state the schedule timing must leave as it found it"""
        ams = [self.fp.max_exp_avg_sq] if self.fp.max_exp_avg_sq is not None else []
        # (the averaged weights with their counters, and the rate word a device schedule writes in every step)
        extra = [] if self.fp.ema is None else [self.fp.ema, self.fp.ema_state]
        if getattr(self, "_sched_rec", None) is not None:
            extra.append(self.lr_dev)
        return [self.fp.flat, self.fp.exp_avg, self.fp.exp_avg_sq, self.fp.step, self.fp.grad_full] + ams + extra

    def _choose_schedule(self):
        """time the two captured schedules on the real step (state saved and restored around it) and keep the faster one.  Data
        parallel: the timing runs replay the graphs only -- no collective, no update -- so a rank whose timing differs (or whose
        side streams misbehave) cannot mispair all-reduces with its peers; the DECISION is then agreed on (MIN over ranks)"""
        snap = _Snapshot(self._state() + _dropout_states(self.net))
        tp = _time_schedule(lambda: self._replay_plain(exchange=False), self.device, *self.TIMING)
        ts = _time_schedule(lambda: self._replay_side(exchange=False), self.device, *self.TIMING)
        bad = self.side.sync_timeouts_now() != self.side.seen
        snap.restore()
        if bad:
            # hand-offs timed out while the side schedule was being timed: the state is restored, the schedule is not used
            self.side.acknowledge()
        torch.cuda.synchronize(self.device)
        self.schedule_times = (tp, ts)
        self._use_side = self.sync.all_true(ts < tp and not bad)
        if not self._use_side:
            self._retire_side_graphs()     # the plain graph won: the side graphs (and their raw HIP executables) are released


class _AveragedWeights:
    """Trainer.averaged_weights(): fp.flat <-> fp.ema exchanged around the block (n3d_swap_f32), host-visible points on both sides"""

    def __init__(self, trainer):
        self.tr = trainer

    def _swap(self):
        tr = self.tr
        K.swap_f32(tr.fp.flat, tr.fp.ema)
        tr._averaged = not tr._averaged

    def __enter__(self):
        tr = self.tr
        if tr._averaged:
            raise K.N3DError("averaged_weights(): already inside the block")
        tr.check_sync()
        if int(tr.fp.ema_state[0].item()) == 0:
            raise K.N3DError("averaged_weights(): no update has been averaged yet")
        self._swap()
        tr.sync_to_module()       # (padded twin: the user's module sees the averaged parameters too)
        return tr

    def __exit__(self, *exc):
        self._swap()
        self.tr.check_sync()
        return False


class Trainer(_GraphTrainer):
    """One searched-net (or any model built from nas_3d_unet_amd ops) training step.

    step(x, t): x (B,4,S,S,S), t (B,3,S,S,S) fp32 device tensors -> loss (0-d device tensor,
    no host sync).  With graph=True the first call captures, later calls replay.
    n_buckets >= 2 (data parallel only): bucketed gradient exchange overlapped with backward, see the module docstring."""

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, graph=True, process_group=None,
                 n_buckets=None, params=None, comm=None, storage=None, side_wgrad=None, optimizer="adam", optim_args=None,
                 grad_clip=None, loss=None, schedule=None, ema=None):
        self.optim = _optim_spec(optimizer, lr, betas, eps, optim_args)
        if schedule is not None and not isinstance(schedule, _LRSchedule):
            raise TypeError("schedule must be a PolyLR or a CosineLR (got %s)" % type(schedule).__name__)
        if ema is not None and not isinstance(ema, EMA):
            raise TypeError("ema must be an EMA (got %s)" % type(ema).__name__)
        self.schedule, self.ema = schedule, ema
        self._averaged = False       # inside averaged_weights(): fp.flat holds the averaged model, fp.ema the training weights
        super().__init__(model, model, lr, betas, eps, graph, process_group, side_wgrad, loss)
        self.net = model      # the module whose kernels run (the model itself, or its padded twin)
        if self._twin is not None:
            from . import unet as _unet
            tw = self.net = self._twin.twin
            tw.forward_loss = lambda x, t, smooth=1e-6, _tw=tw, loss=None: _unet.run_loss(_tw, x, t, None, smooth, loss=loss)
        # side_wgrad: the weight-gradient kernels of the C in {4, 8} levels -- nothing on the backward chain waits for them -- are
        # queued during the backward walk and launched on a SIDE HIP stream at a few cut points (cell boundaries), as separately
        # launched graphs tied to the main chain by events; the streams join once, in front of the slab reduction + Adam.  (Round 3:
        # two per-SAMPLE chains measured no gain -- batching already is that overlap -- while the step's DAG has this slack:
        # profiles/r03_two_chain_probe.log, profiles/r03_seg_overlap.log.)  A replayed side schedule is re-timed every 256 steps and
        # the trainer falls back to the plain graph if it degrades (e.g. another library created hardware queues and the two
        # streams are time-sliced): _side_verdict
        self._capturing_side = False
        self._bracket_now = False    # this step's replay is bracketed with events ...
        self._watch = None           # ... which are read at the start of the next step
        self._recheck = 0            # 1: a slow sample is measured again at the next step
        self._slow_run = 0           # slow samples in a row
        self._static_loss = None
        if storage is not None:
            from . import unet as _unet
            _unet.set_storage(self.net, storage)   # "bf16": bf16 activation storage on the HBM-bound levels (BASELINE configs[4])
        plist = list(params) if params is not None else list(self.net.parameters())
        self.fp = FlatParams(plist, self.device)
        self._pad_mask = None
        if self._twin is not None:
            # gradients of the twin's PADDED parameter entries are not zero (GroupNorm couples a padded channel to its group) and Adam would
            # move them by lr per step: they are masked in front of every update, so the padded entries stay exactly 0
            # (AdaBound / AdaBoundW as well, with weight_decay != 0 too: a masked entry has g = 0 and p = 0, so g' = wd * p = 0,
            # m stays 0, the step r * m is 0 whatever the clamp gives, and the decoupled decay takes wd * 0 off it)
            self._pad_mask = _pad_mask_for(self._twin, self.model, self.fp, self.device)
        if self.optim.amsbound:
            self.fp.ensure_amsbound()
        self._clip = _GradClip(grad_clip, self.device) if grad_clip is not None else None
        if n_buckets is None:
            n_buckets = int(os.environ.get("N3D_DP_BUCKETS", "1"))
        self.n_buckets = max(1, n_buckets)
        self.ctx = K.StepContext(self.device)  # batched weight packing + deferred wgrad reductions
        self.lr_dev = torch.full((1,), float(lr), dtype=torch.float32, device=self.device)  # read by the Adam kernel
        self._one = torch.ones((), dtype=torch.float32, device=self.device)
        self.scheduler = _plateau_for(self, "lr", "set_lr")  # train.py:50: ReduceLROnPlateau(factor=0.5)
        self._sched_rec = None
        if self.schedule is not None:
            # a per-update rule computed on the device in front of every optimiser launch (it writes lr_dev): the plateau rule
            # and a per-update rule would fight over that one word, so there is no plateau scheduler
            self.scheduler = None
            self._sched_rec = self.schedule.record(float(lr), self.device)
        if self.ema is not None:
            self.fp.ensure_ema()
        # (a weight-gradient stream of its own lets the side stream run data gradients of the C <= 8 cells inline: fused.SIDE_PAIRS_BWD)
        self._init_side(comm, wgrad_stream=_fused.SIDE_PAIRS_BWD)
        # the bucketed, overlapped exchange rides on the side-stream schedule (a closed bucket is reduced and sent from the
        # weight-gradient stream); without one the exchange is a single bucket behind the step
        self._buckets = self._bucket_plan() if (self.dp_path and self.n_buckets > 1 and self.side is not None) else None
        if self._buckets is not None:
            self.side.tail_inline = ()      # every weight-gradient group on ONE stream: a closed bucket's slabs are reduced there
            self.sync.ranges = [r for _, r in self._buckets]
        self.sync.broadcast(self.fp.flat)

    # -- subject-level inference -------------------------------------------------------------------
    def predictor(self, patch=64, batch=8, no_patch=False):
        """a predict.SubjectPredictor (prediction.py:64-170 on the device) on the module this trainer's step trains -- its padded
        twin, its storage configuration -- behind a host-visible point (check_sync()).  Its captured forward packs the weights
        inside the graph, so a predictor made once goes on predicting with the weights as later steps leave them.
        no_patch=True (the reference's predict(no_patch=True)): a predict.ImagePredictor on the same module -- one forward per subject
        on the whole padded image; patch and batch do not apply."""
        from .predict import ImagePredictor, SubjectPredictor
        self.check_sync()
        if no_patch:
            return ImagePredictor(self.model, graph=self.use_graph, _net=self.net, _padded=self._twin is not None)
        return SubjectPredictor(self.model, patch, batch, graph=self.use_graph, _net=self.net, _padded=self._twin is not None)

    # -- bucket plan ------------------------------------------------------------------------------
    def _bucket_plan(self):
        """[(cell index whose backward completes the bucket (-1 = the stems, i.e. the end), (begin, end) flat range)] in issue
        order, or None when the model is not a stems / down_cells / up_cells / last_conv net with a fusable head.
        Backward finishes the head first, then the cells last to first, then the stems, and `model.parameters()` lists
        stems, cells, head -- so what is complete after cell k is the TAIL of the flat buffer starting at cell k's first
        parameter.  Bucket j closes at the first point of the backward walk where at least thresholds[j] of the gradient
        bytes are complete; the last bucket closes at the end."""
        m = self.net
        if not all(hasattr(m, a) for a in ("stem0", "stem1", "down_cells", "up_cells", "last_conv")):
            return None
        off = {id(p): (o, o + (p.numel() + 3) // 4 * 4) for p, o in zip(self.fp.params, self.fp.offsets)}
        cells = list(m.down_cells) + list(m.up_cells)
        order = [m.stem0, m.stem1] + cells + [m.last_conv]
        spans, pos = [], 0
        for mod in order:
            ps = list(mod.parameters())
            if not ps or any(id(q) not in off for q in ps):
                return None
            lo, hi = min(off[id(q)][0] for q in ps), max(off[id(q)][1] for q in ps)
            if lo != pos:
                return None          # not the contiguous stems / cells / head order: keep the single bucket
            spans.append((lo, hi))
            pos = hi
        total = self.fp.numel
        if pos != total:
            return None
        n = self.n_buckets
        thresholds = [0.85] if n == 2 else [0.4 + (0.92 - 0.4) * j / (n - 2) for j in range(n - 1)]
        plan, end, j = [], total, 0
        for k in reversed(range(len(cells))):
            if j >= len(thresholds):
                break
            start = spans[2 + k][0]
            if (total - start) / total >= thresholds[j] and start < end and k > 0:
                plan.append((k, (start, end)))
                end = start
                j += 1
        plan.append((-1, (0, end)))
        return plan if len(plan) > 1 else None

    # -- pieces ---------------------------------------------------------------------------------
    def _fwd_bwd(self, x, t):
        with K.step_context(self.ctx):
            self._prepare_loss(t)
            self.ctx.pack_all()            # one launch packs every conv weight for this step
            loss = _loss_of(self.net, self.loss_fn, x, t)
            with _fused.switched(REUSE_GRAD_OUTPUT=True):   # this backward is all ours (no hooks, no retain)
                loss.backward(self._one)  # seed gradient kept resident: no fill launch per step
            self.ctx.flush_final()         # one launch finishes every weight-gradient reduction
        if not self.ctx.frozen:
            self.ctx.freeze()              # first pass only recorded which weights / layouts are needed
        return loss.detach()

    def _pipeline(self, x, t, cell_hook):
        """forward + loss + backward WITHOUT autograd: fused.NetFn and head.HeadDiceFn / HeadLossFn are called directly, so the backward walk
        is one Python function on this thread and can hand over work on the way: cell_hook(k) is called when the backward of cell k
        (-1: the stems, i.e. the end) has been launched."""
        from . import head as _head, programs as _P
        m = self.net
        plan = getattr(m, "_net_plan", None)
        if not _fused.current(plan):
            plan = m._net_plan = _fused.net_plan(m, supernet=False)
        op = m.last_conv[0]
        with torch.no_grad(), K.step_context(self.ctx):
            phi = K.target_sdt(t) if isinstance(self.loss_fn, BoundaryLoss) else None     # at the start of the step, on the main chain
            self.ctx.pack_all()
            nctx = _Ctx((False, False) + (False,) * 4 + (True,) * len(plan.params))
            with _fused.switched(PLANAR_OUT=_fused.PLANAR_LAST):     # (_direct_ok: the head is the fused one)
                body = _fused.NetFn.forward(nctx, plan, x, None, None, None, None, *plan.params)
            gate = _P.draw_gate(op.dropout, op.training, *_head.feat_shape(body), body.device)
            hctx = _Ctx((False, False, True, False, True, True))
            hctx.skip_p = True        # the step returns the loss only: the head does not write the probabilities
            if phi is not None:
                hctx = _Ctx((False, False, False, True, False, True, True))
                hctx.skip_p = True
                loss, _ = _head.HeadBndFn.forward(hctx, gate, self.loss_fn, phi, body, t, op.conv.weight, op.conv.bias)
                dbody = _head.HeadBndFn.backward(hctx, self._one, None)[3]
            elif isinstance(self.loss_fn, TverskyBCELoss):
                loss, _ = _head.HeadLossFn.forward(hctx, gate, self.loss_fn, body, t, op.conv.weight, op.conv.bias)
                dbody = _head.HeadLossFn.backward(hctx, self._one, None)[2]
            else:
                loss, _ = _head.HeadDiceFn.forward(hctx, gate, float(self.loss_fn.smooth), body, t, op.conv.weight, op.conv.bias)
                dbody = _head.HeadDiceFn.backward(hctx, self._one, None)[2]
            with _fused.switched(REUSE_GRAD_OUTPUT=True, CELL_DONE_HOOK=cell_hook):
                _fused.NetFn.backward(nctx, dbody)
        if not self.ctx.frozen:
            self.ctx.freeze()
        return loss

    def _direct_ok(self):
        """can the step run as the autograd-free pipeline (a stems / cells / fusable-head net with a loss the head forms)?"""
        from . import head as _head
        m = self.net
        return (_fused.WHOLE_NET and isinstance(self.loss_fn, (WeightedDiceLoss, TverskyBCELoss, BoundaryLoss)) and not hasattr(m, "kernel")
                and all(hasattr(m, a) for a in ("stem0", "stem1", "down_cells", "up_cells", "last_conv"))
                and _head.fusable(m.last_conv, torch.empty((1, m.last_conv[0].conv.weight.shape[1], 1, 1, 1), device="meta")))

    def _side_ok(self):
        return super()._side_ok() and self._direct_ok()

    def _side_pass(self, x, t):
        """the autograd-free pipeline on two streams (SideSchedule): every deferrable weight-gradient launch is queued and handed to
        the side stream at the cuts of the backward walk (live), and the off-chain pieces of the net itself run there inline
        (fused.SIDE_FWD / SIDE_BWD).  Forward and backward run on this thread, so one arena covers both.  Returns the loss."""
        sd = self.side
        sd.begin_pass()
        with sd.forward_mode(), sd.backward_mode(), sd.deferring():
            cut_hook = _fused.CELL_DONE_HOOK          # (the deferring's: a cut of the weight-gradient queue at every cell boundary)
            if self._buckets is None:
                return self._pipeline(x, t, cell_hook=cut_hook)
            # bucketed exchange (data parallel) on device flags: a bucket that the backward walk has completed is closed on the
            # weight-gradient stream (SideSchedule.close_bucket) and all-reduced THERE, under the rest of the backward; the last
            # bucket (the head of the flat buffer, with the hand-off flag in front) goes out behind the tail, on the step's stream
            closes = {k: j for j, (k, _) in enumerate(self._buckets[:-1])}

            def hook(k):
                cut_hook(k)
                j = closes.get(k)
                if j is not None:
                    sd.close_bucket(lambda: self._bucket_closed(j))
            return self._pipeline(x, t, cell_hook=hook)

    def _bucket_closed(self, j):
        """bucket j is complete on the weight-gradient stream: while the streams are being captured the stream's graph is cut here
        (the all-reduce is launched between the segments at replay), eagerly the all-reduce goes out now"""
        sd = self.side
        if self._capturing_side:
            sd.split_wstream_capture()
        else:
            with torch.cuda.stream(sd.wstream):
                self.sync.reduce_range(j)

    def _side_step_eager(self, x, t):
        loss = self._side_pass(x, t)
        self.side.launch_side(redirect=True)
        self.side.finish()
        return loss

    def _allreduce_last(self):
        """bucketed exchange on flags: the buckets closed during the backward walk are on their way (weight-gradient stream, joined
        by the tail); the last one -- with the hand-off flag in front of it -- goes out here, on the step's stream"""
        if self.sync.active:
            K.guard_flag(self.side.ptr(1), self.side.ptr(4), self.fp.grad_full.data_ptr())
            self.sync.reduce_range(len(self.sync.ranges) - 1)

    def _update(self, loss=None):
        if self._pad_mask is not None:
            self.fp.grad.mul_(self._pad_mask)
        # grad_clip: the norm of the gradient the optimiser is about to see (slabs reduced, padded entries masked, ranks averaged)
        coef = self._clip.launch(self.fp.grad, 1.0 / self.world) if self._clip is not None else None
        if self._sched_rec is not None:
            K.lr_schedule(self.fp.step, self._sched_rec, self.lr_dev)      # the rate of THIS update, from the updates applied so far
        self.fp.update(self.optim, self.lr, 1.0 / self.world, self.lr_dev, self._guard(loss, self.sync), coef)
        if self.ema is not None:
            K.ema_step(self.fp.ema, self.fp.flat, self.ema.decay, self.fp.step, self.fp.ema_state)    # (a withheld update: skipped on the device)

    @property
    def grad_norm(self):
        """0-d device tensor: the global gradient norm of the last step as clip_grad_norm_ returns it (None without grad_clip).
        Written by the step's own launches; reading it here costs no sync"""
        return self._clip.out[0] if self._clip is not None else None

    def set_lr(self, lr):
        """new learning rate for the following steps (also inside an already captured graph).  With a schedule: its BASE rate (one
        device fill of the schedule record, between replays); lr_dev keeps the rate of the last issued step"""
        self.lr = float(lr)
        if self._sched_rec is not None:
            self._sched_rec[1:2].fill_(self.lr)
        else:
            self.lr_dev.fill_(self.lr)

    def _step(self, *batch):
        if self._averaged:
            raise K.N3DError("step() inside averaged_weights(): the flat buffer holds the averaged model, not the training weights")
        return super()._step(*batch)

    def averaged_weights(self):
        """`with tr.averaged_weights():` -- evaluate(), predictor(...).predict(...), metrics.score_set(...) and model.state_dict()
        see the averaged model (train.EMA): the contents of fp.flat and fp.ema are exchanged in place on entry (one launch, no
        allocation; every captured graph packs the weights from fp.flat at replay) and exchanged back on exit, so the training
        weights return bit for bit.  check_sync() on entry and on exit; step() inside the block raises."""
        if self.ema is None:
            raise K.N3DError("averaged_weights(): this trainer was built without ema=EMA(...)")
        return _AveragedWeights(self)

    def _eager(self, x, t, allow_side=True):
        """allow_side=False: single stream whatever the trainer was built with.  The side-stream schedule ties its streams together
        with device-side waits, and anything that makes the HOST wait for the device in the middle of a pass (the caching allocator
        returning memory to the driver when a new shape does not fit its cache, for one) leaves those waits spinning until their
        time-out; a replayed graph allocates nothing, an eager pass on a shape seen for the first time may."""
        if allow_side and self._side_ok() and (self._side_explicit or self.use_graph):
            loss = self._side_step_eager(x, t)
            if self.dp_path:
                if self._buckets is not None:
                    self._allreduce_last()
                else:
                    self._exchange(self.sync)
        else:
            loss = self._fwd_bwd(x, t)
            if self.dp_path:
                self._exchange(self.sync)
        self._update(loss)
        return loss

    # -- capture and replay -----------------------------------------------------------------------
    def _warm_up(self, sided):
        if sided:
            self._side_step_eager(*self._static)
        if not (sided and self._side_force):
            self._fwd_bwd(*self._static)

    def _capture_plain(self):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):  # RCCL's watchdog thread may touch the runtime meanwhile
            self._static_loss = self._fwd_bwd(*self._static)
            if not self.dp_path:
                self._update(self._static_loss)
        self._graph = g

    def _side_passes(self):
        return [(self._captured_side_pass, self._update)]

    def _captured_side_pass(self):
        self._capturing_side = True     # (_bucket_closed: a closed bucket cuts the weight-gradient stream's graph)
        try:
            return self._side_pass(*self._static)
        finally:
            self._capturing_side = False

    def _replay(self):
        if not self._use_side:
            self._replay_plain()
            return self._static_loss
        if self._bracket_now:
            # every 256th STEP (counted by step() on every path: a rank that ran an eager step for an odd-shaped last batch, or
            # recaptured, still counts it) is bracketed with events; the verdict on that sample is taken at the start of the next step
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            self._replay_side()
            e1.record()
            self._watch = (e0, e1)
        else:
            self._replay_side()
        return self._side_losses[0]

    def _replay_side(self, exchange=True):
        # three graphs, no host-side cross-stream dependency: the streams meet through device flags (SideSchedule)
        # (the side graph goes first: its device-side waits are then in place when the main chain reaches its cuts, also when the
        # host is slower at launching than the GPU at running, e.g. under a profiler)
        g_main, side_exec, g_tail = self._side_graphs[0]
        nseg = self._side_wsegs
        if nseg <= 1:
            self.side.raw_replay(side_exec)
            g_main.replay()
            g_tail.replay()
            if self.dp_path and exchange:
                self._exchange(self.sync)
                self._update(self._side_losses[0])
            return
        # bucketed exchange on flags: the weight-gradient stream's graph comes in segments, bucket j's all-reduce between segment j
        # and j + 1 on that stream (no host-side dependency: the segments wait for the chain's flags on the device)
        head, wsegs = side_exec[:-nseg], side_exec[-nseg:]
        self.side.raw_replay(head + wsegs[:1])
        g_main.replay()
        for j in range(1, nseg):
            if exchange:
                with torch.cuda.stream(self.side.wstream):
                    self.sync.reduce_range(j - 1)
            self.side.raw_replay(wsegs[j:j + 1])
        g_tail.replay()
        if exchange:
            self._allreduce_last()
            self._update(self._side_losses[0])

    def _replay_plain(self, exchange=True):
        self._graph.replay()
        if self.dp_path and exchange:
            self._exchange(self.sync)
            self._update(self._static_loss)

    def _side_verdict(self):
        """start of a step, one step after a bracketed one: the trainer checks the time-outs of the device-side waits (raises) and the
        bracketed step's GPU time against the plain schedule's measured time -- a side schedule that has become slower than the plain
        graph is dropped.  Data parallel: the verdict is COLLECTIVE, and its place in the stream of collectives is a function of the
        STEP COUNT alone (every rank calls step() the same number of times, whatever path each step takes on a rank; a rank without
        a sample -- its bracketed step ran eagerly -- votes "fast"): one tiny all-reduce of "my sample was fast", issued before
        anything of this step.  A rank that retired its side schedule on its own would go on with another fp32 summation order than
        its peers and the replicas would drift apart bit by bit."""
        sd = self.side
        n = self._n_steps
        due, self._bracket_now = self._bracket_now, False
        # is THIS step a bracketed one?  (uniform over the ranks: the step count, or a re-check every rank agreed on one step ago)
        want = sd is not None and self._use_side and (n % 256 == 0 or self._recheck > 0)
        if want:
            self._recheck = 0
        if sd is not None and self._use_side and due:
            fast, ms = True, None
            if self._watch is not None:
                e0, e1 = self._watch
                self._watch = None
                e1.synchronize()
                sd.check()      # (the per-step poll() has seen a withheld update long before; this also catches a time-out whose
                                # step was not followed by an update yet)
                ms = e0.elapsed_time(e1)
                fast = self.schedule_times is None or ms * 1e-3 <= 1.5 * self.schedule_times[0] + 2e-4
            slow = not (self.sync.all_true(fast) if self.dp_path else fast)
            # ONE slow sample proves nothing -- the bracket also holds whatever the host did between the three graph launches (a
            # 100 000-step soak dropped a healthy schedule on a single 3.5 ms sample): a slow sample is measured again, three in a row
            # retire the schedule
            self._slow_run = (self._slow_run + 1) if slow else 0
            self._recheck = 1 if (slow and self._slow_run < 3) else 0
            if self._slow_run >= 3:
                import warnings
                warnings.warn("nas_3d_unet_amd: the side-stream schedule degraded (%s ms per step on this rank against %.2f ms for the plain "
                              "graph, three samples in a row%s); falling back to the plain graph"
                              % ("%.2f" % ms if ms is not None else "?", self.schedule_times[0] * 1e3, " on at least one rank" if self.dp_path else ""))
                self._use_side = False
                if self._graph is None:      # ("force": no plain graph was captured -- the next step captures one)
                    torch.cuda.synchronize(self.device)
                    self._retire_side_graphs()
                    self._side_retired = True
                    self._static = None
        self._bracket_now = bool(want and self._use_side)


class SearchTrainer(_GraphTrainer):
    """Supernet search step, first-order DARTS as in the reference (search.py:211-238):
    architecture pass on the validation batch (Adam on the four alpha matrices), then weight pass on the
    training batch (Adam on the kernel weights); both Adam instances use torch defaults (search.py:103-104).

    Exact-equivalent savings over the reference: the architecture pass does not compute weight gradients
    (the reference computes and discards them, search.py:231) and the weight pass does not compute alpha
    gradients -- requires_grad is switched per pass, so the corresponding kernels are simply not launched."""

    N_INPUTS = 4
    TIMING = (1, 3)

    def __init__(self, shell, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, graph=True, process_group=None, comm=None, side_wgrad=None,
                 optimizer="adam", optim_args=None, grad_clip=None, loss=None):
        # loss: both passes, the architecture pass and the weight pass (search.py:224-226,233-235 call one loss function)
        # optimizer / optim_args / grad_clip: the weight pass (search.py:236-238: the commented clip line sits in front of
        # optim_kernel.step()); the alphas stay on Adam (search.py:103)
        self.optim = _optim_spec(optimizer, lr, betas, eps, optim_args)     # (an SGD / AdamW spec object: the weight pass, as well)
        super().__init__(shell, shell.kernel, lr, betas, eps, graph, process_group, side_wgrad, loss)
        # a kernel net with channel counts that are not multiples of 4: the shell's own alphas around its zero-padded twin
        self.net = shell if self._twin is None else _TwinShell(shell, self._twin.twin)
        # the weight pass queues its weight-gradient kernels for the side stream (SideSchedule); the architecture pass has none
        self._side_active = True     # _pass: use the side stream (when there is one; off while the plain graphs are captured)
        self.side_forward = True    # ... also for the off-chain edges of the forward passes
        self.side_backward = True   # ... and for the preprocess-fed edges of the backward passes
        # which preprocess-fed edges the side stream takes in the backward: the second input's only (round 4; "01" = both until then --
        # since the node levels' phases are single launches the chain absorbs the first input's terms in its own, wider, launches
        # and the side stream's last node level -- which the chain waits for at the end of every cell -- is half as long:
        # architecture pass 5.45 -> 5.25 ms, profiles/r04_search_phases.log)
        self.side_backward_inputs = (1,)
        self.side_backward_weight = ()      # (weight pass without a weight-gradient stream of its own: none)
        self._replays = 0            # replays of the side schedule: every 256th is followed by a check()
        self._losses = None
        self.kparams = list(shell.kernel.parameters()) if self._twin is None else list(self._twin.twin.parameters())
        self.aparams = list(shell.alphas())
        self.fp = FlatParams(self.kparams, self.device)
        self._pad_mask = _pad_mask_for(self._twin, shell.kernel, self.fp, self.device) if self._twin is not None else None
        if self.optim.amsbound:
            self.fp.ensure_amsbound()
        self._clip = _GradClip(grad_clip, self.device) if grad_clip is not None else None
        self.aflat, self.agrad, aoffs = flatten_params(self.aparams, self.device)
        self.a_m = torch.zeros_like(self.aflat)
        self.a_v = torch.zeros_like(self.aflat)
        self.a_step = K.step_counter(self.device) if self.device.type == "cuda" else torch.zeros(1, dtype=torch.int32, device=self.device)
        # the alphas' Adam state in the shape checkpoint.adam_state_dict reads (optim_shell, search.py:103)
        self.afp = types.SimpleNamespace(params=self.aparams, offsets=aoffs, exp_avg=self.a_m, exp_avg_sq=self.a_v, step=self.a_step)
        self._one = torch.ones((), dtype=torch.float32, device=self.device)
        self.ctx = K.StepContext(self.device)
        # the weight pass' weight-gradient stream (219 launches) ends ~0.5 ms behind the chain: every other group of the walk's last
        # eleven goes to the inline side stream instead, which has little else to do in the backward (weight pass 5.57 + 0.51 ->
        # 5.78 + 0.09 ms; more groups there slow the chain by more than they take off the tail: profiles/r04_search_phases.log,
        # DESIGN.md section 5).  384 slab jobs per weight pass: reducing most of them early shrinks the tail 0.23 -> 0.15 ms
        self._init_side(comm, wgrad_stream=True, tail_inline=(1, 3, 5, 7, 9, 11), early_finalize=6)
        # two learning rates (search.py:103-106): alphas ("shell") and kernel weights, each on its own plateau schedule
        self.lr_shell, self.lr_kernel = float(lr), float(lr)
        self.lr_shell_dev = torch.full((1,), float(lr), dtype=torch.float32, device=self.device)
        self.lr_kernel_dev = torch.full((1,), float(lr), dtype=torch.float32, device=self.device)
        self.shell_scheduler = _plateau_for(self, "lr_shell", "set_shell_lr")
        self.kernel_scheduler = _plateau_for(self, "lr_kernel", "set_kernel_lr")
        # data parallel: two exchanges per step -- the alpha gradients (180 floats) after the architecture pass,
        # the kernel-weight gradients (27.4 MB, sync_kernel) after the weight pass; weights and alphas broadcast once from rank 0
        self.sync_alpha = GradSync(self.agrad, self.pg, 1, None, comm, header=self.agrad._n3d_full)
        self.sync_kernel.broadcast(self.fp.flat)
        self.sync_kernel.broadcast(self.aflat)

    def _eval_net(self):
        """the kernel net (or its padded twin) under the shell's current softmaxed alphas (search.py:154: validate() runs the shell)"""
        return (self.model.kernel if self._twin is None else self._twin.twin), self.model._soft

    @property
    def sync_kernel(self):
        """the kernel-weight exchange (the base class' `sync`, which also carries the schedule agreements)"""
        return self.sync

    def set_shell_lr(self, lr):
        self.lr_shell = float(lr)
        self.lr_shell_dev.fill_(self.lr_shell)

    def set_kernel_lr(self, lr):
        self.lr_kernel = float(lr)
        self.lr_kernel_dev.fill_(self.lr_kernel)

    def _pass(self, x, t, arch, update=True, pack=True, side="inline"):
        """pack=False: the conv weights were packed by the pass before and have not changed since (the weight pass of a step
        follows the architecture pass, which only moves the alphas).
        side (weight pass with a SideSchedule): "inline" = queue the weight-gradient launches, then issue them on the side stream
        and join (eager use); "main" = only the main-stream part (the graph capture issues launch_side / finish itself)."""
        for p in self.kparams:
            p.requires_grad_(not arch)
        for p in self.aparams:
            p.requires_grad_(arch)
        if arch:
            self.agrad.zero_()  # alpha gradients arrive through autograd accumulation (softmax backward)
        # with a side stream BOTH passes use it: the forward of either pass runs the off-chain edges of every supernet cell there
        # (fused._run_forward_side), the weight pass also queues its weight-gradient launches for it
        sided = self._side_active and self._side_ok()
        from . import programs as _P
        _P.PASS_TAG = "arch" if arch else "weight"
        with K.step_context(self.ctx):
            self._prepare_loss(t)
            if pack:
                self.ctx.pack_all()
            if sided and self.side_forward:
                with self.side.forward_mode():
                    loss = _loss_of(self.net, self.loss_fn, x, t)
            else:
                loss = _loss_of(self.net, self.loss_fn, x, t)
            # architecture pass: the side stream takes both preprocess-fed edges of every node (6 of a cell's 9: 7.8 -> 6.9 ms);
            # weight pass: it already carries every weight gradient -- with both edge sets on top the pass takes 9.6 instead of
            # 8.1 ms, with one 9.1 -- so its backward stays on one stream
            # -- unless they run on a stream of their own (SideSchedule.split): then the weight pass does the same, 8.1 -> 7.1 ms
            bwd_inputs = self.side_backward_inputs if (arch or (sided and self.side.split)) else self.side_backward_weight
            with _fused.switched(REUSE_GRAD_OUTPUT=True):
                with (self.side.backward_mode(bwd_inputs) if (sided and self.side_backward and bwd_inputs) else contextlib.nullcontext()):
                    if sided and not arch:
                        with self.side.deferring():
                            loss.backward(self._one)
                    else:
                        loss.backward(self._one)  # seed gradient kept resident: no fill launch per step
            if not sided:
                self.ctx.flush_final()
        if sided and side == "main":
            return loss.detach()
        if sided:
            self.side.launch_side(redirect=True)
            self.side.finish()
        if not self.ctx.frozen and not arch:
            self.ctx.freeze()
        if update:
            self._update(arch, loss.detach())
        return loss.detach()

    def _update(self, arch, loss=None):
        """exchange (data parallel) + Adam of the pass that just ran; guarded: a timed-out hand-off (on any rank) withholds it"""
        sync = self.sync_alpha if arch else self.sync_kernel
        if self.dp_path:
            self._exchange(sync)
        guard = self._guard(loss, sync)
        if arch:
            K.adam_step(self.aflat, self.agrad, self.a_m, self.a_v, self.a_step, self.lr_shell, self.betas[0], self.betas[1], self.eps,
                        grad_scale=1.0 / self.world, lr_dev=self.lr_shell_dev, guard=guard)
        else:
            if self._pad_mask is not None:
                self.fp.grad.mul_(self._pad_mask)       # (padded twin: the padded entries' gradients are not zero -- see Trainer)
            coef = self._clip.launch(self.fp.grad, 1.0 / self.world) if self._clip is not None else None
            self.fp.update(self.optim, self.lr_kernel, 1.0 / self.world, self.lr_kernel_dev, guard, coef)

    @property
    def grad_norm(self):
        """0-d device tensor: the kernel weights' global gradient norm of the last weight pass (None without grad_clip)"""
        return self._clip.out[0] if self._clip is not None else None

    def _both(self, x, t, vx, vt, update=True):
        la = self._pass(vx, vt, True, update)
        lw = self._pass(x, t, False, update, pack=False)   # same weights as the architecture pass just packed
        return la, lw

    @contextlib.contextmanager
    def _one_stream(self):
        was, self._side_active = self._side_active, False
        try:
            yield
        finally:
            self._side_active = was

    def _eager(self, x, t, val_x, val_t, allow_side=True):
        """allow_side=False: on ONE stream (Trainer._eager says why)"""
        if allow_side:
            return self._both(x, t, val_x, val_t)
        with self._one_stream():
            return self._both(x, t, val_x, val_t)

    # -- capture and replay -----------------------------------------------------------------------
    def _warm_up(self, sided):
        self._both(*self._static, update=False)

    def _capture_plain(self):
        x, t, vx, vt = self._static
        with self._one_stream():
            if self.dp_path:
                # one graph per pass (forward + backward only); the exchange and Adam of each pass run eagerly behind it
                pool = torch.cuda.graph_pool_handle()
                ga, gw = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
                with torch.cuda.graph(ga, pool=pool, capture_error_mode="thread_local"):
                    la = self._pass(vx, vt, True, update=False)
                with torch.cuda.graph(gw, pool=pool, capture_error_mode="thread_local"):
                    lw = self._pass(x, t, False, update=False, pack=False)
                self._losses, self._graph = (la, lw), (ga, gw)
            else:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, capture_error_mode="thread_local"):  # RCCL's watchdog thread may touch the runtime meanwhile
                    self._losses = self._both(x, t, vx, vt)
                self._graph = g

    def _side_passes(self):
        x, t, vx, vt = self._static
        return [(lambda: self._pass(vx, vt, True, update=False, side="main"), lambda loss: self._update(True, loss)),
                (lambda: self._pass(x, t, False, update=False, pack=False, side="main"), lambda loss: self._update(False, loss))]

    def _state(self):
        return super()._state() + [self.aflat, self.agrad._n3d_full, self.a_m, self.a_v, self.a_step]

    def _replay(self):
        if not self._use_side:
            self._replay_plain()
            return self._losses
        self._replay_side()
        self._replays += 1
        if self._replays % 256 == 0:
            self.side.check()
        return self._side_losses

    def _replay_side(self, exchange=True):
        for arch, loss, (g_main, side_exec, g_tail) in zip((True, False), self._side_losses, self._side_graphs):
            self.side.raw_replay(side_exec)      # first: see Trainer._replay_side
            g_main.replay()
            g_tail.replay()
            if self.dp_path and exchange:
                self._update(arch, loss)

    def _replay_plain(self, exchange=True):
        """the plain graph; data parallel one graph per pass, each followed by its exchange and update"""
        if not self.dp_path:
            self._graph.replay()
            return
        for arch, loss, g in zip((True, False), self._losses, self._graph):
            g.replay()
            if exchange:
                self._update(arch, loss)
