#!/usr/bin/env python3
"""One batch of anchor-making problems shaped like the long-read stage's: reads of 15 kbp off haplotype walks of the 1 Mbp graph with substitutions, their
seeds from the device's own minimizer seeding (pipeline.seed_long_reads under GIRAFFE_LONG_READ_POLICY), their gapless extensions from vgk_gapless_extend
without trimming; `distinct` reads made, repeated up to `problems`.  Prints one JSON line: the three kernel groups' device ms and the wall time of
vgk_extension_anchors, and — labelled as what it is, the CHECKER — the host shim's vgh_extension_anchors on 16 host threads for the same input.
--extender oracle: the extensions come from the CPU oracle's vgk_gapless_extend instead of the engine's (the measured call is the same).
    python tools/extension_anchors_time.py [--problems 4000] [--distinct 200] [--read-len 15000] [--extender engine|oracle]"""
import argparse, ctypes, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vg_amd import capi, pipeline, workloads

ap = argparse.ArgumentParser()
ap.add_argument("--problems", type=int, default=4000); ap.add_argument("--distinct", type=int, default=200); ap.add_argument("--read-len", type=int, default=15000)
ap.add_argument("--extender", choices=("engine", "oracle"), default="engine")
args = ap.parse_args()
eng = capi.Engine(capi.Scoring.simple(1, 4, 6, 1, 5))
wl = workloads.ExtensionAnchorsWorkload(min(args.distinct, args.problems), seed=3, read_len=args.read_len, graph_bp=1_000_000, k=31, w=50)
index = eng.haplo_index(wl.nodes, wl.threads)
extend_with = None
if args.extender == "oracle":
    ora = capi.Engine(capi.Scoring.simple(1, 4, 6, 1, 5), lib=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "libvgoracle.so"))
    extend_with = (ora, ora.haplo_index(wl.nodes, wl.threads))
base = pipeline.extension_anchors(eng, index, wl.problems(eng, index), extend_with=extend_with)
statuses, counts = np.unique(base["gapless_status"], return_counts=True)
# ---- the batch: the distinct problems repeated (offsets shifted, the arrays they index shared)
d = len(base["seed_off"]) - 1; reps = -(-args.problems // d)
ns = np.diff(base["seed_off"].astype(np.int64)); ne = np.diff(base["ext_off"].astype(np.int64))
seed_off = np.concatenate([[0], np.cumsum(np.tile(ns, reps)[:args.problems])]).astype(np.uint64); ext_off = np.concatenate([[0], np.cumsum(np.tile(ne, reps)[:args.problems])]).astype(np.uint64)
seeds = np.tile(base["seeds"], reps)[:int(seed_off[-1])]; ext = np.tile(base["extensions"], reps)[:int(ext_off[-1])]; full = np.tile(base["full_length"], reps)[:args.problems]
wall = []; dev = []
for rep in range(4):
    t = time.perf_counter()
    out = eng.extension_anchors(index, seed_off, seeds, ext_off, ext, full, base["nodes"], base["mismatches"])
    wall.append(time.perf_counter() - t); dev.append(eng.extension_anchors_last_ms())
olen = np.repeat(np.array([len(s) for s in wl.nodes], dtype=np.uint32), 2)
t = time.perf_counter()
rc, ref = capi.extension_anchors_call(pipeline._host_lib().vgh_extension_anchors, (ctypes.c_void_p(olen.ctypes.data), ctypes.c_uint64(len(olen))), 1, 4, 0, 4, seed_off, seeds, ext_off, ext, full,
                                      base["nodes"], base["mismatches"], tail=(ctypes.c_int(16),))
shim_s = time.perf_counter() - t
print(json.dumps(dict(extender=args.extender, gapless_statuses={int(a): int(b) for a, b in zip(statuses, counts)}, problems=args.problems, distinct=d, read_len=args.read_len, seeds=int(len(seeds)), seeds_per_problem=float(len(seeds)) / args.problems, extensions=int(len(ext)),
                      mismatches_per_extension=float(ext["n_mismatches"].mean()) if len(ext) else 0.0, anchors=int(len(out["anchors"])), full_length_problems=int((out["status"] != 0).sum()),
                      kernel_ms=dict(seed_anchors_sort=dev[-1][0], extension_seed_lists=dev[-1][1], anchors=dev[-1][2]), kernel_ms_all=dev,
                      call_wall_s_median_warm=float(np.median(wall[1:])), call_wall_s_all=wall, checker_shim_16_threads_s=shim_s,
                      identical_to_checker=bool(rc == 0 and all(out[f].tobytes() == ref[f].tobytes() for f in ("anchor_off", "anchors", "origins", "rep_off", "represented", "status"))))))
