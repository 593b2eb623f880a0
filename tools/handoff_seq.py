"""The launch sequence of the 64^3 train step's side-stream schedule per stream, from the C-ABI calls recorded while the trainer captures it: how many
of the main chain's launches are flag launches (n3d_sync_*), how many of those sit next to each other (profiles/r06_handoff_seq.log), which entry
point follows each signal on its stream -- the launch that carries the signal in its entry (n3d_entry_signal_arm) -- and how many stand-alone signal
launches are left (profiles/entry_signal_ab.log).  N3D_ENTRY_SIGNALS=0: every signal a launch of its own."""
import os, sys, collections, argparse
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch, bench
from kernel_table import Recorder
from nas_3d_unet_amd import kernels as K, searched
from nas_3d_unet_amd.train import Trainer, SearchTrainer, reserve_side_streams
ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=64)
ap.add_argument("--dtype", default="f32", choices=["f32", "bf16"])
ap.add_argument("--workload", default="train", choices=["train", "search"], help="search: the supernet's search step (two passes with hand-offs per step)")
args = ap.parse_args()
print("workload %s, 4x%d^3, %s" % (args.workload, args.size, args.dtype))
dev = torch.device("cuda", 0)
reserve_side_streams(dev)
torch.manual_seed(1234)
xn, tn = bench.synthetic_batch(2, args.size, 1)
x, t = bench.to_patch_layout(torch.from_numpy(xn).to(dev)), torch.from_numpy(tn).to(dev)
if args.workload == "search":
    from nas_3d_unet_amd import nas
    C_ = bench.CFG
    net = nas.ShellNet(C_["in_channels"], C_["init_n_kernels"], C_["out_channels"], C_["depth"], C_["n_nodes"], False, C_["channel_change"]).to(dev); net.train()
    tr = SearchTrainer(net, graph=True, side_wgrad="force")
    vxn, vtn = bench.synthetic_batch(2, args.size, 4321)
    batch = (x, t, bench.to_patch_layout(torch.from_numpy(vxn).to(dev)), torch.from_numpy(vtn).to(dev))
else:
    net = searched.SearchedNet(4, 4, 3, 4, 3, True, searched.Genotype(**bench.G_CONV)).to(dev); net.train()
    tr = Trainer(net, graph=True, storage="bf16" if args.dtype == "bf16" else None)
    batch = (x, t)
c0 = K.entry_signal_counts()
with Recorder() as r:
    tr.step(*batch)
torch.cuda.synchronize()
c1 = K.entry_signal_counts()
print("entry signals while the step was captured: %d carried in a kernel's entry, %d launched stand-alone by the library" % (c1[0] - c0[0], c1[1] - c0[1]))
NOT_LAUNCHES = ("n3d_entry_signal_arm", "n3d_entry_signal_flush", "n3d_entry_signal_pending", "n3d_entry_signal_counts")
calls = r.calls
print("calls recorded:", len(calls))
# passes are separated by n3d_pack_batch (one per forward); take the LAST pass that contains sync calls
starts = [i for i, (n, a) in enumerate(calls) if n == "n3d_pack_batch"] + [len(calls)]
withsync = []
for a, b in zip(starts[:-1], starts[1:]):
    seg = calls[a:b]
    ns = sum(1 for n, _ in seg if n.startswith("n3d_sync") or n == "n3d_entry_signal_arm")
    print("pass at", a, "len", b - a, "sync calls", ns)
    if ns: withsync.append(seg)
# the captured step: its last pass with hand-offs (search: the last two, architecture pass + weight pass)
best = sum(withsync[-2:], []) if args.workload == "search" else withsync[-1]
def sp(args):
    v = args[-1]
    return getattr(v, "value", v)
streams = collections.OrderedDict()
for n, a in best:
    if a and n not in NOT_LAUNCHES:
        streams.setdefault(sp(a), []).append(n)
for s, names in streams.items():
    sync = [n for n in names if n.startswith("n3d_sync")]
    print("stream", s, "launches", len(names), "sync", len(sync), collections.Counter(sync))
# the entry point that follows each signal on its own stream: the launch that can carry the signal in its entry (n3d_entry_signal_arm)
from kernel_table import describe, _shape_text
full = collections.OrderedDict()
for n, a in best:
    if a and n not in NOT_LAUNCHES[1:]:
        full.setdefault(sp(a), []).append((n, a))
for s, seq in full.items():
    if not isinstance(s, int):
        continue
    for kind in ("n3d_sync_signal", "n3d_entry_signal_arm"):
        succ, shapes, last = collections.Counter(), collections.Counter(), 0
        for k, (n, a) in enumerate(seq):
            if n != kind:
                continue
            nxt = [(n2, a2) for n2, a2 in seq[k + 1:] if n2 != "n3d_entry_signal_arm"]
            if not nxt:
                last += 1
                continue
            n2, a2 = nxt[0]
            succ[n2] += 1
            if not n2.startswith("n3d_sync"):
                shapes[(n2, _shape_text(describe(n2, a2)[0]))] += 1
        what = "stand-alone signal launches" if kind == "n3d_sync_signal" else "signals armed for the next launch"
        print("stream", s, what + ":", sum(succ.values()) + last, "-- followed by:", dict(succ), "-- last launch of the stream:", last)
        for (n2, sh), c in sorted(shapes.items()):
            print("    %2d x %s  %s" % (c, n2, sh))
main = max(streams.items(), key=lambda kv: len(kv[1]))[1]
# adjacency on the main stream
adj = collections.Counter()
for p, q in zip(main[:-1], main[1:]):
    if p.startswith("n3d_sync") and q.startswith("n3d_sync"):
        adj[(p, q)] += 1
print("adjacent sync pairs on the main stream:", dict(adj))
runs = []; cur = 0
for n in main:
    if n.startswith("n3d_sync"): cur += 1
    else:
        if cur: runs.append(cur)
        cur = 0
print("runs of consecutive sync launches on main:", collections.Counter(runs))
print("main sequence (S=signal launch W=wait 2=wait2 .=other; armed signals are not launches and do not appear):")
print("".join("S" if n == "n3d_sync_signal" else "W" if n == "n3d_sync_wait" else "2" if n == "n3d_sync_wait2" else "." for n in main))
