#!/usr/bin/env python3
"""4 000 reads of 15 kbp on the workload of profiles/r06/long_read_seeding.json: the three-call path with the host choice on 16 threads against the fused call."""
import os, sys, time, json
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vg_amd import capi, pipeline, workloads
n = 4000; L = 15000
g = workloads.VariationGraph(ref_len=50818468)
rng = np.random.default_rng(7)
comp = workloads._comp_table()
reads = np.empty((n, L), dtype=np.uint8)
for i in range(n):
    hseq = g.haps[int(rng.integers(0, 2))][0]; a = int(rng.integers(0, len(hseq) - L)); r = hseq[a:a + L]
    reads[i] = comp[r[::-1]] if rng.random() < 0.5 else r
sub = rng.random(reads.shape) < 0.005
reads[sub] = workloads.ACGT[rng.integers(0, 4, int(sub.sum()))]
off = np.arange(n + 1, dtype=np.uint64) * L
eng = capi.Engine(capi.Scoring.simple(1, 4, 6, 1, 5))
threads = [(2 * np.nonzero(hap_pos >= 0)[0]).astype(np.uint32) for _, hap_pos in g.haps]
mi = eng.minimizer_index((g.node_len, g.seq), threads)
k = 29; flat = reads.ravel()
res = {}
for mode in ("host", "device"):
    wall = []; dev = []
    for rep in range(7):
        t = time.perf_counter(); out = pipeline.seed_long_reads(eng, mi, flat, off, k, threads=16, choice=mode); wall.append(time.perf_counter() - t)
        dev.append(eng.minimizer_choose_last_ms())
    res[mode] = dict(wall_s_median_of_5_warm=float(np.median(wall[2:])), wall_s_all=wall, choose_kernels_ms_median=float(np.median(dev[2:])), calls=getattr(eng, "find_seeds_calls", 0),
                     minimizers=len(out["minimizers"]), taken=int(out["take"].sum()), seeds=len(out["seeds"]))
    res[mode + "_take"] = out["take"]
res["identical_take"] = bool((res.pop("host_take") == res.pop("device_take")).all())
# the fused call with room known beforehand (one call, no retry)
wall = []
for rep in range(6):
    t = time.perf_counter(); eng.minimizer_find_seeds(mi, pipeline.GIRAFFE_LONG_READ_POLICY, flat, off, cap_m=res["device"]["minimizers"], cap_s=res["device"]["seeds"]); wall.append(time.perf_counter() - t)
res["device_sized"] = dict(wall_s_median_of_5_warm=float(np.median(wall[1:])), calls=eng.find_seeds_calls, choose_kernels_ms=eng.minimizer_choose_last_ms())
print(json.dumps(res))
