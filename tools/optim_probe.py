"""probe: what the optimiser options cost the captured 64^3 fp32 train step (batch 2, G_conv, as bench.py's headline run).

Four configurations of this tree -- default (Adam), adabound, adam + grad_clip, adabound + grad_clip -- and, with --parent DIR (a
checkout of the parent commit with its library built), the default configuration of that tree, which has none of the options.
Every measurement runs in a process of its own; the trees alternate, --repeats times, and the spread of the parent's repeats is the
yardstick for "the default path did not change".  Usage:

    python tools/optim_probe.py [--parent DIR] [--repeats 3] [--steps 200] [--log profiles/optim_probe.log]
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = {
    "default": {},
    "adabound": dict(optimizer="adabound"),
    "adam+clip": dict(grad_clip=5.0),
    "adabound+clip": dict(optimizer="adabound", grad_clip=5.0),
    "adaboundw+ams+clip": dict(optimizer="adaboundw", optim_args=dict(amsbound=True, weight_decay=1e-2), grad_clip=5.0),
}


def child(root, names, steps, size):
    sys.path.insert(0, root)
    import torch
    import bench
    from nas_3d_unet_amd import searched
    from nas_3d_unet_amd.train import Trainer, reserve_side_streams
    dev = torch.device("cuda")
    reserve_side_streams(dev)
    for name in names:
        torch.manual_seed(1234)
        net = searched.SearchedNet(4, 4, 3, 4, 3, True, searched.Genotype(**bench.G_CONV)).to(dev)
        net.train()
        tr = Trainer(net, graph=True, **CONFIGS[name])
        xn, tn = bench.synthetic_batch(2, size, 1234)
        x, t = bench.to_patch_layout(torch.from_numpy(xn).to(dev)), torch.from_numpy(tn).to(dev)
        for _ in range(20):
            tr.step(x, t)
        x, t = tr.input_buffers()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            loss = tr.step(x, t)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / steps * 1e3
        tr.check_sync()
        print(json.dumps({"config": name, "ms_per_step": round(ms, 4), "params": tr.fp.numel, "loss": round(float(loss), 6),
                          "schedule": "side" if getattr(tr, "_use_side", False) else "plain"}), flush=True)
        del tr, net


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None, help="(internal) tree whose package is imported")
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--parent", default=None)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.configs.split(","), args.steps, args.size)
    rows = []

    def run(tag, root, configs):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", root, "--configs", configs, "--steps", str(args.steps), "--size", str(args.size)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise SystemExit("%s: child failed with status %d\n%s" % (tag, r.returncode, r.stderr[-2000:]))
        for line in r.stdout.splitlines():
            if line.startswith("{"):
                rows.append(dict(json.loads(line), tree=tag))
                print(rows[-1], flush=True)

    for _ in range(args.repeats):
        if args.parent:
            run("parent", os.path.abspath(args.parent), "default")
        run("this", HERE, args.configs)
    out = ["# tools/optim_probe.py: captured %d^3 fp32 train step (batch 2, G_conv), %d steps per figure, %d alternating repeats, one process each"
           % (args.size, args.steps, args.repeats), "# tree config ms/step per repeat | median | min..max | schedule | parameters"]
    for tree in ("parent", "this"):
        for name in CONFIGS:
            ms = [r["ms_per_step"] for r in rows if r["tree"] == tree and r["config"] == name]
            if ms:
                r0 = [r for r in rows if r["tree"] == tree and r["config"] == name][0]
                out.append("%-7s %-20s %s | %.4f | %.4f..%.4f | %s | %d" % (tree, name, " ".join("%.4f" % v for v in ms), sorted(ms)[len(ms) // 2],
                                                                            min(ms), max(ms), r0["schedule"], r0["params"]))
    text = "\n".join(out) + "\n"
    print(text)
    if args.log:
        with open(args.log, "w") as f:
            f.write(text)


if __name__ == "__main__":
    sys.exit(main())
