"""probe: what the training-recipe options cost the captured fp32 train step (batch 2, G_conv, as bench.py's headline run) at 64^3 and
128^3: default arguments, SGD (Nesterov), AdamW, a device schedule, averaged weights, and all three together.

All configurations of this tree live in ONE process, each with its captured step graph; they are timed in alternating rounds
(--rounds rounds of --steps replays each) and the figure of a configuration is the median of its rounds, so drift of the machine
hits every configuration alike.  With --parent DIR (a checkout of the parent commit with its library built) the default configuration
of that tree is timed the same way in a process of its own, before and after.  The launch counts are the libn3d entry points one
eager single-stream step calls (every one of them launches; torch's own launches -- the input copies -- are the same for all).
Usage:

    python tools/recipe_probe.py [--parent DIR] [--sizes 64,128] [--rounds 5] [--steps 50] [--log profiles/recipe_probe.log]
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_CALLS = ("n3d_sgd_step", "n3d_adamw_step", "n3d_lr_schedule", "n3d_ema_step", "n3d_swap_f32")


def configs(train):
    if not hasattr(train, "SGD"):        # (the parent tree)
        return {"default": {}}
    sgd = lambda: train.SGD(momentum=0.99, nesterov=True, weight_decay=3e-5)
    return {
        "default": {},
        "sgd": dict(lr=1e-2, optimizer=sgd()),
        "adamw": dict(optimizer=train.AdamW(weight_decay=1e-2)),
        "adam+poly": dict(schedule=train.PolyLR(total_steps=100000, warmup_steps=100)),
        "adam+ema": dict(ema=train.EMA(0.999)),
        "sgd+poly+ema": dict(lr=1e-2, optimizer=sgd(), schedule=train.PolyLR(total_steps=100000), ema=train.EMA(0.999)),
    }


class Calls:
    """the libn3d entry points called while the block runs"""

    def __init__(self, _lib):
        self._lib, self.names = _lib, []

    def __enter__(self):
        real, names = self._lib.load(), self.names

        class Proxy:
            def __getattr__(self, name):
                fn = getattr(real, name)
                if not name.startswith("n3d_"):
                    return fn

                def counted(*a):
                    names.append(name)
                    return fn(*a)
                return counted

        self._real, self._lib._lib = real, Proxy()
        return self

    def __exit__(self, *exc):
        self._lib._lib = self._real


def child(root, names, rounds, steps, size):
    sys.path.insert(0, root)
    import torch
    import bench
    from nas_3d_unet_amd import _lib, searched, train
    dev = torch.device("cuda")
    train.reserve_side_streams(dev)
    cfgs = {k: v for k, v in configs(train).items() if k in names}

    def make(name, **kw):
        torch.manual_seed(1234)
        net = searched.SearchedNet(4, 4, 3, 4, 3, True, searched.Genotype(**bench.G_CONV)).to(dev)
        net.train()
        return train.Trainer(net, **dict(cfgs[name], **kw))

    xn, tn = bench.synthetic_batch(2, size, 1234)
    x, t = bench.to_patch_layout(torch.from_numpy(xn).to(dev)), torch.from_numpy(tn).to(dev)
    counts = {}
    for name in cfgs:        # launch counts: one eager single-stream step
        tr = make(name, graph=False, side_wgrad=False)
        tr.step(x, t)
        with Calls(_lib) as c:
            tr.step(x, t)
        torch.cuda.synchronize()
        calls = [n for n in c.names if n != "n3d_last_error"]
        counts[name] = (len(calls), [n for n in calls if n.startswith(NEW_CALLS)])
        del tr
    trainers = {}
    for name in cfgs:
        tr = make(name, graph=True)
        for _ in range(20):
            tr.step(x, t)
        trainers[name] = (tr, tr.input_buffers())
    torch.cuda.synchronize()
    ms = {name: [] for name in cfgs}
    for _ in range(rounds):
        for name, (tr, (xs, ts)) in trainers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                loss = tr.step(xs, ts)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / steps * 1e3)
    for name, (tr, _) in trainers.items():
        tr.check_sync()
        print(json.dumps({"config": name, "size": size, "ms": [round(v, 4) for v in ms[name]], "params": tr.fp.numel,
                          "schedule": "side" if getattr(tr, "_use_side", False) else "plain", "calls": counts[name][0],
                          "new_calls": counts[name][1]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None, help="(internal) tree whose package is imported")
    ap.add_argument("--configs", default="default,sgd,adamw,adam+poly,adam+ema,sgd+poly+ema")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--sizes", default="64,128")
    ap.add_argument("--size", type=int, default=64, help="(internal)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.configs.split(","), args.rounds, args.steps, args.size)
    rows = []

    def run(tag, root, cfg, size):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", root, "--configs", cfg, "--rounds", str(args.rounds), "--steps", str(args.steps),
               "--size", str(size)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit("%s: child failed with status %d\n%s" % (tag, r.returncode, r.stderr[-2000:]))
        for line in r.stdout.splitlines():
            if line.startswith("{"):
                rows.append(dict(json.loads(line), tree=tag))
                print(rows[-1], flush=True)

    sizes = [int(s) for s in args.sizes.split(",")]
    for size in sizes:
        if args.parent:
            run("parent", os.path.abspath(args.parent), "default", size)
        run("this", HERE, args.configs, size)
        if args.parent:
            run("parent", os.path.abspath(args.parent), "default", size)
    med = lambda v: sorted(v)[len(v) // 2]
    out = ["# tools/recipe_probe.py: captured fp32 train step (batch 2, 4 channels, G_conv); per configuration %d alternating rounds of %d replays, "
           "all configurations of a tree in one process" % (args.rounds, args.steps),
           "# size tree config | median ms/step | min..max of the rounds | x this tree's default | schedule | libn3d calls per eager step | new calls"]
    for size in sizes:
        base = med([v for r in rows if r["tree"] == "this" and r["config"] == "default" and r["size"] == size for v in r["ms"]])
        for tree in ("parent", "this"):
            for name in args.configs.split(","):
                sel = [r for r in rows if r["tree"] == tree and r["config"] == name and r["size"] == size]
                if sel:
                    ms = [v for r in sel for v in r["ms"]]
                    out.append("%d^3 %-6s %-13s | %.4f | %.4f..%.4f | %.4f | %s | %d | %s" % (size, tree, name, med(ms), min(ms), max(ms), med(ms) / base,
                                                                                             sel[0]["schedule"], sel[0]["calls"], " ".join(sel[0]["new_calls"]) or "-"))
    if not args.parent:
        out.append("# no --parent given: the parent commit's default step was NOT timed in this run")
    text = "\n".join(out) + "\n"
    print(text)
    if args.log:
        with open(args.log, "w") as f:
            f.write(text)


if __name__ == "__main__":
    sys.exit(main())
