#!/usr/bin/env python3
"""Long reads against ONE resident graph, two ways on one library (the shape of bench.py's wide leg, which this does not touch): 2 000 reads of
1.1-9 kbp, half pinned X-drop, half LOCAL, all with tracebacks, over a chain of 32-base nodes with SNP bubbles, about 1 Mbp.
  (a) vgk_gssw_align on the explicit induced subgraphs — the route a caller had before: packed on one host thread, whole op slots copied back;
  (b) vgk_gssw_align_windows — each read a window of the resident graph, packed on the device, written ops only copied back.
Two warm-up calls each, then the median and spread of --calls calls.  Prints one JSON line, then tools/kernel_registers.py's rows for the new kernels.
    python tools/wide_windows_timing.py [--reads 2000] [--calls 5] [--ref 1000000]"""
import argparse, ctypes, json, os, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vg_amd import capi

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=2000); ap.add_argument("--calls", type=int, default=5); ap.add_argument("--ref", type=int, default=1_000_000)
args = ap.parse_args()
rng = np.random.default_rng(97)
acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
ref = acgt[rng.integers(0, 4, args.ref)]
# ---- the graph: 32-base nodes, now and then a SNP bubble (reference allele first); node_pos = the reference offset a node begins at
nodes, preds, node_pos, segments, at = [], [], [], [], 0
while at < len(ref):
    ln = min(32, len(ref) - at)
    after_bubble = len(nodes) >= 3 and len(nodes[-1]) == 1 and len(nodes[-2]) == 1 and preds[-1] == preds[-2]
    segments.append(len(nodes)); node_pos.append(at)
    nodes.append(ref[at:at + ln].tobytes().decode()); preds.append([len(nodes) - 3, len(nodes) - 2] if after_bubble else ([len(nodes) - 2] if len(nodes) > 1 else []))
    at += ln
    if rng.random() < 0.05 and at + 33 < len(ref):
        a = len(nodes) - 1
        nodes.append(chr(ref[at])); preds.append([a]); node_pos.append(at)
        nodes.append("ACGT"[(b"ACGT".index(ref[at]) + 1) % 4]); preds.append([a]); node_pos.append(at)
        at += 1
node_pos = np.array(node_pos + [len(ref)]); segments = np.array(segments)
node_len = np.array([len(s) for s in nodes], dtype=np.uint32)
seq = np.frombuffer("".join(nodes).encode(), dtype=np.uint8).copy()
pred_off = np.concatenate([[0], np.cumsum([len(p) for p in preds])]).astype(np.uint32)
pred_idx = np.array([q for p in preds for q in p], dtype=np.uint32)
# ---- the reads, each a window; the same problems as explicit induced subgraphs
reads, first, count, flags, explicit = [], [], [], [], []
for i in range(args.reads):
    L = int(rng.integers(1100, 9000))
    xdrop = i % 2 == 1
    a = int(segments[int(rng.integers(0, np.searchsorted(node_pos[segments], len(ref) - L - 700)))])
    start = int(node_pos[a]) + (0 if xdrop else 100)                       # pinned at the window's first base: the read starts there
    b = int(np.searchsorted(node_pos[:-1], start + L + 200, side="left"))
    read = ref[start:start + L].copy()
    sub = rng.random(L) < 0.01
    read[sub] = acgt[rng.integers(0, 4, int(sub.sum()))]
    read = np.delete(read, np.nonzero(rng.random(L) < 0.002)[0])
    fl = (capi.VGK_XDROP_PINNED if xdrop else capi.VGK_GSSW_LOCAL) | capi.VGK_GSSW_TRACEBACK
    reads.append(read); first.append(a); count.append(b - a); flags.append(fl)
    explicit.append(dict(read=read.tobytes().decode(), nodes=nodes[a:b], preds=[[q - a for q in preds[v] if q >= a] for v in range(a, b)], flags=fl, pinning=None, max_gap=40))
read_off = np.concatenate([[0], np.cumsum([len(r) for r in reads])])
first = np.array(first); count = np.array(count)
col = np.concatenate([[0], np.cumsum(node_len, dtype=np.int64)])
ws = capi.WindowSet(np.concatenate(reads), read_off, first, count, np.array(flags, dtype=np.uint32), np.full(len(reads), 40), cols=col[first + count] - col[first])
ps = capi.ProblemSet.from_lists(explicit)

eng = capi.Engine(capi.Scoring.simple(1, 4, 6, 1, 5))
g = eng.graph(node_len, seq, pred_off, pred_idx)
n = ws.n
cap = int(np.diff(read_off).sum() + ws.cols.sum() + 4 * n)
res_a = np.zeros(n, dtype=capi.RESULT_DT); ops_a = np.zeros(cap, dtype=capi.OP_DT); res_b = np.zeros(n, dtype=capi.RESULT_DT); ops_b = np.zeros(cap, dtype=capi.OP_DT)
written = ctypes.c_size_t()


def call_a():
    t = time.perf_counter()
    rc = eng.lib.vgk_gssw_align(eng.h, ps.ptr, n, res_a.ctypes.data, ops_a.ctypes.data, cap, ctypes.byref(written))
    assert rc == 0, rc
    return dict(wall_ms=(time.perf_counter() - t) * 1e3, fill_ms=eng.wide_last(0), walk_ms=eng.wide_last(1), launches=eng.wide_last(4), ops=written.value)


def call_b():
    t = time.perf_counter()
    rc = eng.lib.vgk_gssw_align_windows(eng.h, g.h, ws.reads.ctypes.data_as(ctypes.c_char_p), ws.reads.size, ws.array.ctypes.data, n, res_b.ctypes.data, ops_b.ctypes.data, cap, ctypes.byref(written))
    assert rc == 0, rc
    return dict(wall_ms=(time.perf_counter() - t) * 1e3, pack_ms=eng.align_windows_last(0), fill_ms=eng.align_windows_last(1), walk_ms=eng.align_windows_last(2),
                wide=eng.align_windows_last(3), sub_batches=eng.align_windows_last(4), op_bytes=eng.align_windows_last(5), ops=written.value)


def series(fn):
    runs = [fn() for _ in range(2 + args.calls)][2:]
    out = {k: float(np.median([r[k] for r in runs])) for k in runs[0]}
    for k in ("wall_ms", "fill_ms", "walk_ms", "pack_ms"):
        if k in runs[0]:
            out[k + "_min_max"] = [float(min(r[k] for r in runs)), float(max(r[k] for r in runs))]
    return out


a = series(call_a); b = series(call_b)
same = all((res_a[f] == res_b[f]).all() for f in ("status", "score", "end_node", "end_offset", "end_read", "first_offset", "n_ops"))
for i in range(n):
    if not same:
        break
    x = ops_a[res_a["ops_begin"][i]:res_a["ops_begin"][i] + res_a["n_ops"][i]].view(np.uint64); y = ops_b[res_b["ops_begin"][i]:res_b["ops_begin"][i] + res_b["n_ops"][i]].view(np.uint64)
    same = bool((x == y).all())
rows = np.diff(read_off) + (np.arange(n) % 2 == 1)
print(json.dumps(dict(reads=n, graph_nodes=len(nodes), graph_bases=int(col[-1]), cells=int((rows * ws.cols).sum()), calls=args.calls,
                      explicit_vgk_gssw_align=a, windows_vgk_gssw_align_windows=b, identical=same, failed=int((res_b["status"] != 0).sum()),
                      mean_score_per_base=float((res_b["score"] / np.diff(read_off)).mean()),
                      op_slot_bytes_explicit=int((np.diff(read_off) + ws.cols + 2).sum() * 8), op_bytes_windows=b["op_bytes"])))
sys.stdout.flush()
subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_registers.py"), os.path.join(ROOT, "vg_amd", "libvgamd.so"), "wwin_"])
