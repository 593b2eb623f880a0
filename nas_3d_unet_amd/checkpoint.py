"""Checkpoint / genotype interoperability with the reference; host logic only.

The reference saves `torch.save({...})` dictionaries (train.py:85-93: epoch, history, model_param, optim, scheduler,
best_loss; search.py:166-176 adds geno_count, optim_shell / optim_kernel, shell_scheduler / kernel_scheduler) and reads
them back in check_resume (train.py:52-67; search.py:108-127); the genotype travels as a pickled `(str(gene), count)`
that is `eval`ed (search.py:189-194; train.py:36-38).  Module state-dicts need no conversion (same keys and shapes).
What does need one is the optimizer: the trainers keep Adam's moments in flat buffers with ONE step counter, torch's
Adam keeps per-parameter tensors -- `adam_state_dict` / `load_adam_state_dict` translate both ways, and the plateau
schedulers export / import torch's ReduceLROnPlateau field names.  A trainer built with optimizer="adabound" / "adaboundw" writes the
state_dict() layout of the reference's adabound.py classes instead (`adabound_state_dict`) and records its optimiser's name under
"optimizer" ("optimizer_kernel" in a search checkpoint); loading state another optimiser wrote raises ValueError.  A trainer built
with optimizer=train.SGD(...) / train.AdamW(...) writes torch.optim.SGD's / AdamW's own state_dict() layout and records its name
the same way; with ema= the dictionary gains "ema" (n_averaged and the averaged parameters in model_param's layout), with schedule=
the "scheduler" entry holds the schedule's fields.  Files of trainers built without these arguments are key for key what they were.
"""
from __future__ import annotations

import pickle

import torch

from .genotype import Genotype


# ------------------------------------------------------------------------------------------------ Adam
def _entries(fp, twin=None, real=None):
    """[(offset in the flat buffers, stored shape, name | None)] in the order torch.optim.Adam(real.parameters()) numbers its parameters.
    A trainer of a net with odd channel counts keeps the moments of the net's zero-padded TWIN (unet.PaddedTwin): its flat buffers are
    walked in the REAL module's parameter order and every moment goes through twin.extract / twin.embed_tensor, so the checkpoint holds
    the reference's shapes (a torch / reference checkpoint of the same net loads, and the other way round)."""
    if twin is None:
        return [(o, p.shape, None) for p, o in zip(fp.params, fp.offsets)]
    off = {id(p): (o, p.shape) for p, o in zip(fp.params, fp.offsets)}
    tp = dict(twin.twin.named_parameters())
    out = []
    for n, _ in real.named_parameters():
        if n in tp and id(tp[n]) in off:
            o, shape = off[id(tp[n])]
            out.append((o, shape, n))
    if len(out) != len(fp.params):
        raise ValueError("padded twin: %d of the trainer's %d parameters have no counterpart in the module" % (len(fp.params) - len(out), len(fp.params)))
    return out


def adam_state_dict(fp, lr, betas=(0.9, 0.999), eps=1e-8, twin=None, real=None):
    """torch.optim.Adam(params).state_dict() equivalent of a train.FlatParams (params in `fp.params` order; with a padded twin: in
    `real.parameters()` order and the reference's shapes)."""
    step = int(fp.step.item())
    state = {}
    ents = _entries(fp, twin, real)
    for i, (o, shape, name) in enumerate(ents):
        n = int(torch.Size(shape).numel())
        if step > 0:
            m, v = fp.exp_avg[o:o + n].view(shape), fp.exp_avg_sq[o:o + n].view(shape)
            if name is not None:
                m, v = twin.extract(name, m), twin.extract(name, v)
            state[i] = {"step": torch.tensor(float(step)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
    group = {"lr": lr, "betas": tuple(betas), "eps": eps, "weight_decay": 0, "amsgrad": False, "maximize": False, "foreach": None,
             "capturable": False, "differentiable": False, "fused": None, "decoupled_weight_decay": False,
             "params": list(range(len(ents)))}
    return {"state": state, "param_groups": [group]}


def load_adam_state_dict(fp, sd, twin=None, real=None):
    """inverse of adam_state_dict; returns the learning rate stored in the checkpoint.
    Limit: the flat Adam keeps ONE step counter, so every parameter with state must be at the same step (true for every
    checkpoint the reference writes: all parameters receive a gradient in every step); otherwise ValueError."""
    steps = set()
    fp.exp_avg.zero_()
    fp.exp_avg_sq.zero_()
    for i, (o, shape, name) in enumerate(_entries(fp, twin, real)):
        st = sd["state"].get(i)
        if st is None:
            continue
        n = int(torch.Size(shape).numel())
        m, v = st["exp_avg"].to(fp.exp_avg.device), st["exp_avg_sq"].to(fp.exp_avg.device)
        if name is not None:     # reference shapes -> the twin's (zeros at the padded entries, which Adam never moves: masked gradients)
            m, v = twin.embed_tensor(name, m, shape), twin.embed_tensor(name, v, shape)
        fp.exp_avg[o:o + n].copy_(m.reshape(-1))
        fp.exp_avg_sq[o:o + n].copy_(v.reshape(-1))
        steps.add(int(float(st["step"])))
    if len(steps) > 1:
        raise ValueError("checkpoint has different Adam step counts per parameter: %s" % sorted(steps))
    fp.step.fill_(steps.pop() if steps else 0)
    return float(sd["param_groups"][0]["lr"])


# ------------------------------------------------------------------------------------------------ AdaBound / AdaBoundW
def _optim_of(trainer):
    """the trainer's train.OptimSpec (a trainer without one runs Adam)"""
    return getattr(trainer, "optim", None)


def adabound_state_dict(fp, optim, lr, twin=None, real=None):
    """state_dict() of the reference's AdaBound / AdaBoundW (adabound.py) for a train.FlatParams: per parameter `step` (an int, as
    the class counts it), `exp_avg`, `exp_avg_sq` and, with amsbound, `max_exp_avg_sq`; the param group holds lr, betas, final_lr,
    gamma, eps, weight_decay, amsbound.  Parameter order and shapes as adam_state_dict."""
    step = int(fp.step.item())
    bufs = [("exp_avg", fp.exp_avg), ("exp_avg_sq", fp.exp_avg_sq)] + ([("max_exp_avg_sq", fp.max_exp_avg_sq)] if optim.amsbound else [])
    state = {}
    ents = _entries(fp, twin, real)
    for i, (o, shape, name) in enumerate(ents):
        n = int(torch.Size(shape).numel())
        if step > 0:
            st = {"step": step}
            for key, buf in bufs:
                t = buf[o:o + n].view(shape)
                st[key] = (twin.extract(name, t) if name is not None else t).clone()
            state[i] = st
    wd = optim.weight_decay
    group = {"lr": lr, "betas": tuple(optim.betas), "final_lr": optim.final_lr, "gamma": optim.gamma, "eps": optim.eps,
             "weight_decay": int(wd) if wd == 0 else wd, "amsbound": optim.amsbound, "params": list(range(len(ents)))}
    return {"state": state, "param_groups": [group]}


def load_adabound_state_dict(fp, optim, sd, twin=None, real=None):
    """inverse of adabound_state_dict; returns the learning rate stored in the checkpoint.  Moments and step are loaded; final_lr,
    gamma, weight_decay, betas and eps stay the trainer's.  A file whose amsbound differs from the trainer's is refused rather than
    half loaded."""
    group = sd["param_groups"][0]
    if "final_lr" not in group:
        raise ValueError("checkpoint's optimizer state is not AdaBound's (param group keys: %s)" % sorted(group))
    if bool(group.get("amsbound", False)) != optim.amsbound:
        raise ValueError("checkpoint was written with amsbound=%s, the trainer runs amsbound=%s" % (group.get("amsbound", False), optim.amsbound))
    if optim.amsbound:
        fp.ensure_amsbound()
    bufs = [("exp_avg", fp.exp_avg), ("exp_avg_sq", fp.exp_avg_sq)] + ([("max_exp_avg_sq", fp.max_exp_avg_sq)] if optim.amsbound else [])
    for _, buf in bufs:
        buf.zero_()
    steps = set()
    for i, (o, shape, name) in enumerate(_entries(fp, twin, real)):
        st = sd["state"].get(i)
        if st is None:
            continue
        n = int(torch.Size(shape).numel())
        for key, buf in bufs:
            t = st[key].to(buf.device)
            if name is not None:     # reference shapes -> the twin's (zeros at the padded entries, which no optimiser here moves)
                t = twin.embed_tensor(name, t, shape)
            buf[o:o + n].copy_(t.reshape(-1))
        steps.add(int(float(st["step"])))
    if len(steps) > 1:
        raise ValueError("checkpoint has different step counts per parameter: %s" % sorted(steps))
    fp.step.fill_(steps.pop() if steps else 0)
    return float(group["lr"])


# ------------------------------------------------------------------------------------------------ SGD / AdamW
def _plain(x):
    """torch writes 0 for a default it was given as the int 0"""
    return int(x) if x == 0 else x


def sgd_state_dict(fp, optim, lr, twin=None, real=None):
    """torch.optim.SGD(params).state_dict() for a train.FlatParams under a train.SGD spec: per parameter `momentum_buffer` (the
    flat exp_avg; no state before the first step or without momentum), group keys lr, momentum, dampening, weight_decay, nesterov
    and torch's flags.  torch's SGD counts no steps; the trainer's counter travels next to the optimiser's name (_record_optimizer)."""
    step = int(fp.step.item())
    state = {}
    ents = _entries(fp, twin, real)
    if step > 0 and optim.momentum != 0:
        for i, (o, shape, name) in enumerate(ents):
            n = int(torch.Size(shape).numel())
            b = fp.exp_avg[o:o + n].view(shape)
            state[i] = {"momentum_buffer": (twin.extract(name, b) if name is not None else b).clone()}
    group = {"lr": lr, "momentum": _plain(optim.momentum), "dampening": _plain(optim.dampening), "weight_decay": _plain(optim.weight_decay),
             "nesterov": optim.nesterov, "maximize": False, "foreach": None, "differentiable": False, "fused": None,
             "params": list(range(len(ents)))}
    return {"state": state, "param_groups": [group]}


def load_sgd_state_dict(fp, optim, sd, step=None, twin=None, real=None):
    """inverse of sgd_state_dict; returns the learning rate stored in the checkpoint.  step: the update count recorded next to the
    state; a file torch's own SGD wrote has none: 1 when it holds momentum buffers (all the kernel asks is whether a first step was
    taken), else 0.  momentum, dampening, weight_decay and nesterov stay the trainer's."""
    group = sd["param_groups"][0]
    if "momentum" not in group or "betas" in group:
        raise ValueError("checkpoint's optimizer state is not SGD's (param group keys: %s)" % sorted(group))
    fp.exp_avg.zero_()
    have = False
    for i, (o, shape, name) in enumerate(_entries(fp, twin, real)):
        b = sd["state"].get(i, {}).get("momentum_buffer")
        if b is None:
            continue
        have = True
        n = int(torch.Size(shape).numel())
        b = b.to(fp.exp_avg.device)
        if name is not None:
            b = twin.embed_tensor(name, b, shape)
        fp.exp_avg[o:o + n].copy_(b.reshape(-1))
    fp.step.fill_(int(step) if step is not None else (1 if have else 0))
    return float(group["lr"])


def adamw_state_dict(fp, optim, lr, twin=None, real=None):
    """torch.optim.AdamW(params).state_dict() for a train.FlatParams under a train.AdamW spec: Adam's per-parameter layout (step,
    exp_avg, exp_avg_sq), the group with the spec's weight_decay and decoupled_weight_decay = True"""
    sd = adam_state_dict(fp, lr, optim.betas, optim.eps, twin, real)
    sd["param_groups"][0].update(weight_decay=_plain(optim.weight_decay), decoupled_weight_decay=True)
    return sd


def load_adamw_state_dict(fp, optim, sd, twin=None, real=None):
    group = sd["param_groups"][0]
    if "betas" not in group or "final_lr" in group:
        raise ValueError("checkpoint's optimizer state is not AdamW's (param group keys: %s)" % sorted(group))
    return load_adam_state_dict(fp, sd, twin, real)


def _optim_state_dict(trainer, fp, lr, twin, real):
    optim = _optim_of(trainer)
    if optim is None or optim.name == "adam":
        return adam_state_dict(fp, lr, trainer.betas, trainer.eps, twin, real)
    if optim.name == "sgd":
        return sgd_state_dict(fp, optim, lr, twin, real)
    if optim.name == "adamw":
        return adamw_state_dict(fp, optim, lr, twin, real)
    return adabound_state_dict(fp, optim, lr, twin, real)


def _load_optim_state_dict(trainer, fp, sd, written_by, twin, real, step=None):
    """written_by: the optimiser name the checkpoint records (files from before the record, and the reference's own Adam
    checkpoints, carry none: "adam"); step: the update count an SGD checkpoint records next to the name"""
    optim = _optim_of(trainer)
    mine = "adam" if optim is None else optim.name
    if written_by != mine:
        raise ValueError("checkpoint's optimizer state was written by %r, this trainer runs %r: build the trainer with optimizer=%r "
                         "(or load with new_lr=True to take the weights only)" % (written_by, mine, written_by))
    if mine == "adam":
        return load_adam_state_dict(fp, sd, twin, real)
    if mine == "sgd":
        return load_sgd_state_dict(fp, optim, sd, step, twin, real)
    if mine == "adamw":
        return load_adamw_state_dict(fp, optim, sd, twin, real)
    return load_adabound_state_dict(fp, optim, sd, twin, real)


# ------------------------------------------------------------------------------------------------ scheduler
_SCHED_FIELDS = ("factor", "patience", "threshold", "cooldown", "eps", "best", "num_bad_epochs", "cooldown_counter", "last_epoch")


def scheduler_state_dict(s):
    """ReduceLROnPlateau.state_dict() field names for a train.PlateauLR"""
    d = {k: getattr(s, k) for k in _SCHED_FIELDS}
    d.update({"mode": "min", "threshold_mode": "rel", "min_lrs": [s.min_lr], "mode_worse": float("inf"), "_last_lr": [s.get_lr()]})
    return d


def load_scheduler_state_dict(s, d):
    for k in _SCHED_FIELDS:
        if k in d:
            setattr(s, k, d[k])
    if "min_lrs" in d:
        s.min_lr = d["min_lrs"][0]


# ------------------------------------------------------------------------------------------------ train.py:85-93 / 52-67
def _checked(trainer):
    """a checkpoint is a host-visible point: a timed-out stream hand-off (whose update was withheld on the device) raises here
    instead of being written out as if the steps since had trained (train.Trainer.check_sync)"""
    chk = getattr(trainer, "check_sync", None)
    if chk is not None:
        chk()


def _twin_of(trainer, real):
    """(twin, real module) of a trainer that trains a padded twin, (None, None) otherwise"""
    tw = getattr(trainer, "_twin", None)
    return (tw, real) if tw is not None else (None, None)


def _record_optimizer(sd, key, trainer):
    """which optimiser wrote the kernel weights' state: AdaBound and AdaBoundW share one layout, so the name goes next to it.  An Adam
    checkpoint stays key for key the reference's (train.py:85-93; search.py:166-176) and carries no record.  SGD's state counts no
    steps (torch's does not), so the trainer's update count goes next to the name, under key + "_step"."""
    optim = _optim_of(trainer)
    if optim is not None and optim.name != "adam":
        sd[key] = optim.name
        if optim.name == "sgd":
            sd[key + "_step"] = int(trainer.fp.step.item())
    return sd


# ------------------------------------------------------------------------------------------------ device schedule / averaged weights
def _trainer_scheduler_state_dict(trainer):
    """the plateau scheduler's fields, or -- a trainer built with schedule= has none -- the schedule's own as a plain dict"""
    sched = getattr(trainer, "schedule", None)
    return scheduler_state_dict(trainer.scheduler) if sched is None else sched.state_dict()


def _check_scheduler_kind(trainer, d):
    """a checkpoint of another schedule kind (a plateau file into a PolyLR trainer, a cosine file into a plateau trainer ..) raises,
    before anything of the optimiser's state is touched"""
    sched = getattr(trainer, "schedule", None)
    mine, theirs = ("plateau" if sched is None else sched.name), d.get("kind", "plateau")
    if mine != theirs:
        raise ValueError("checkpoint's scheduler state is of kind %r, this trainer runs %r (load with new_lr=True to take the weights only)"
                         % (theirs, mine))


def _load_trainer_scheduler(trainer, d):
    """the plateau scheduler's fields; a device schedule has no state beyond its constructor arguments and the step counter"""
    if getattr(trainer, "schedule", None) is None:
        load_scheduler_state_dict(trainer.scheduler, d)


def _flat_views(trainer, buf):
    """{parameter name: the part of `buf` (a flat buffer laid out like trainer.fp.flat) that belongs to it, in the module's shape}"""
    fp = trainer.fp
    tw, _ = _twin_of(trainer, trainer.model)
    off = {id(p): (o, p.shape) for p, o in zip(fp.params, fp.offsets)}
    src = dict((tw.twin if tw is not None else trainer.model).named_parameters())
    out = {}
    for n, _ in trainer.model.named_parameters():
        q = src.get(n)
        if q is not None and id(q) in off:
            o, shape = off[id(q)]
            v = buf[o:o + int(torch.Size(shape).numel())].view(shape)
            out[n] = (tw.extract(n, v) if tw is not None else v, o, shape)
    return out


def ema_state_dict(trainer):
    """{"n_averaged", "params"}: the averaged weights in model_param's layout (the module's state_dict() with every trained
    parameter replaced by its average), loadable into a module of the same net"""
    params = {k: v.clone() for k, v in trainer.model.state_dict().items()}
    for n, (v, _, _) in _flat_views(trainer, trainer.fp.ema).items():
        params[n] = v.clone()
    return {"n_averaged": int(trainer.fp.ema_state[0].item()), "params": params}


def load_ema_state_dict(trainer, d):
    """inverse of ema_state_dict; d None (a checkpoint without averaged weights): averaging starts over at the next update"""
    fp = trainer.fp
    tw, _ = _twin_of(trainer, trainer.model)
    fp.ema.zero_()
    n_averaged = 0
    if d is not None:
        n_averaged = int(d["n_averaged"])
        for n, (_, o, shape) in _flat_views(trainer, fp.ema).items():
            t = d["params"][n].to(fp.ema.device)
            if tw is not None:
                t = tw.embed_tensor(n, t, shape)
            fp.ema[o:o + t.numel()].copy_(t.reshape(-1))
    fp.ema_state.copy_(torch.tensor([n_averaged, int(fp.step.item()), 0], dtype=torch.int32))


def train_state_dicts(trainer, epoch, history, best_loss):
    _checked(trainer)
    sd = {"epoch": epoch, "history": history, "model_param": trainer.model.state_dict(),
          "optim": _optim_state_dict(trainer, trainer.fp, trainer.lr, *_twin_of(trainer, trainer.model)),
          "scheduler": _trainer_scheduler_state_dict(trainer), "best_loss": best_loss}
    if getattr(trainer, "ema", None) is not None:
        sd["ema"] = ema_state_dict(trainer)
    return _record_optimizer(sd, "optimizer", trainer)


def load_train_state_dicts(trainer, sd, new_lr=False):
    """returns (next epoch, history, best_loss) like check_resume"""
    trainer.model.load_state_dict(sd["model_param"])   # parameters are views of the flat buffer: copied in place
    getattr(trainer, "sync_from_module", lambda: None)()   # (a padded twin re-embeds the loaded parameters)
    if not new_lr:
        _check_scheduler_kind(trainer, sd["scheduler"])
        trainer.set_lr(_load_optim_state_dict(trainer, trainer.fp, sd["optim"], sd.get("optimizer", "adam"), *_twin_of(trainer, trainer.model),
                                              step=sd.get("optimizer_step")))
        _load_trainer_scheduler(trainer, sd["scheduler"])
    if getattr(trainer, "ema", None) is not None:
        load_ema_state_dict(trainer, sd.get("ema"))
    return sd["epoch"] + 1, sd["history"], sd["best_loss"]


# ------------------------------------------------------------------------------------------------ search.py:166-176 / 108-127
def search_state_dicts(trainer, epoch, geno_count, history, best_loss):
    """the reference's search checkpoint: two optimizers, two schedulers (the reference stores the KERNEL scheduler under
    both scheduler keys, search.py:174; here each key holds its own scheduler)"""
    _checked(trainer)
    sd = {"epoch": epoch, "geno_count": geno_count, "history": history, "model_param": trainer.model.state_dict(),
          "optim_shell": adam_state_dict(trainer.afp, trainer.lr_shell, trainer.betas, trainer.eps),
          "optim_kernel": _optim_state_dict(trainer, trainer.fp, trainer.lr_kernel, *_twin_of(trainer, trainer.model.kernel)),
          "kernel_scheduler": scheduler_state_dict(trainer.kernel_scheduler),
          "shell_scheduler": scheduler_state_dict(trainer.shell_scheduler), "best_loss": best_loss}
    return _record_optimizer(sd, "optimizer_kernel", trainer)


def load_search_state_dicts(trainer, sd, new_lr=False):
    """returns (next epoch, geno_count, history, best_loss) like search.py's check_resume"""
    trainer.model.load_state_dict(sd["model_param"])   # kernel weights and alphas are views of the flat buffers: copied in place
    getattr(trainer, "sync_from_module", lambda: None)()   # (a padded twin re-embeds the loaded parameters)
    if not new_lr:
        trainer.set_shell_lr(load_adam_state_dict(trainer.afp, sd["optim_shell"]))
        trainer.set_kernel_lr(_load_optim_state_dict(trainer, trainer.fp, sd["optim_kernel"], sd.get("optimizer_kernel", "adam"),
                                                     *_twin_of(trainer, trainer.model.kernel), step=sd.get("optimizer_kernel_step")))
        load_scheduler_state_dict(trainer.shell_scheduler, sd["shell_scheduler"])
        load_scheduler_state_dict(trainer.kernel_scheduler, sd["kernel_scheduler"])
    return sd["epoch"] + 1, sd["geno_count"], sd["history"], sd["best_loss"]


# ------------------------------------------------------------------------------------------------ genotype pickle
def save_genotype(path, gene, count=1):
    """search.py:189-194: pickle of (str(gene), count)"""
    with open(path, "wb") as f:
        pickle.dump((str(gene), count), f)


class _StrTupleUnpickler(pickle.Unpickler):
    """a genotype file holds (str, int): no class needs to be importable, so none is"""

    def find_class(self, module, name):
        raise pickle.UnpicklingError("genotype file references %s.%s: only a (str, count) tuple is accepted" % (module, name))


def load_genotype(path):
    """train.py:36-38 does `eval(pickle.load(f)[0])`; here the pickle may only contain builtin containers / str / int and
    the text is parsed as a literal `Genotype(down=[...], up=[...])` call (ast), never evaluated"""
    import ast
    with open(path, "rb") as f:
        text = _StrTupleUnpickler(f).load()[0]
    try:
        call = ast.parse(text.strip(), mode="eval").body
        if not (isinstance(call, ast.Call) and isinstance(call.func, ast.Name) and call.func.id == "Genotype"):
            raise ValueError
        args = [ast.literal_eval(a) for a in call.args]
        kw = {k.arg: ast.literal_eval(k.value) for k in call.keywords}
        gene = Genotype(*args, **kw)
    except (ValueError, SyntaxError, TypeError):
        raise ValueError("not a Genotype: %r" % (text,))
    return gene
