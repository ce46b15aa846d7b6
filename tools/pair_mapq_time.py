#!/usr/bin/env python
"""What a pair's mapping qualities cost: vgk_pair_mapq on the device against the host shim on 16 threads (profiles/r11_pair_mapq).

    python tools/pair_mapq_time.py pairs [pairs [out.json]]     a million configs[3]-shaped pairs (2 x 150 bp, k = 29, w = 11, one to four candidates a pair)
    python tools/pair_mapq_time.py heavy [pairs [out.json]]     2 000 pairs of 2 000 candidates each: the shape a lane per pair should lose on

One section per process, so that a job can run each under its own time limit.  The reads are random bases (what is timed reads no graph): their
minimizers are listed on the device (vgk_minimizer_list over a small index) and their agglomerations made there, 70 % explored, Illumina-like qualities.
Both forms are timed: caps given (one double per read goes up) and caps made in the call (the mates' sweep first, then the pair kernels).  The engine's
calls are timed host-inclusive (uploads, kernels, the way back): one warm-up, then five calls — smallest, median and largest are reported;
vgk_pair_mapq_last_ms gives the kernels' share of the last call, vgk_pair_mapq_last_kernel_launches the launches it counted.  The shim's vgh_pair_mapq runs on 16 threads, best of two.  Prints one JSON line, and writes it
to out.json when that is given."""
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vg_amd import capi, pipeline, workloads      # noqa: E402

K, W, THREADS, LENGTH = 29, 11, 16, 150


def timed(repeats, call, warm=1):
    for _ in range(warm):
        call()
    times = []
    for _ in range(repeats):
        t = time.perf_counter(); out = call(); times.append((time.perf_counter() - t) * 1e3)
    return {"min": round(min(times), 2), "median": round(float(np.median(times)), 2), "max": round(max(times), 2)}, out


def main():
    section = sys.argv[1] if len(sys.argv) > 1 else "pairs"
    n = {"pairs": 1_000_000, "heavy": 2000}[section]
    if len(sys.argv) > 2:
        n = int(sys.argv[2])
    rng = np.random.default_rng(11)
    per_pair = rng.choice([1, 2, 3, 4], n, p=[0.55, 0.25, 0.12, 0.08]) if section == "pairs" else np.full(n, 2000)
    cand_off = np.concatenate([[0], np.cumsum(per_pair)]).astype(np.uint64); total = int(cand_off[-1])
    pair_of = np.repeat(np.arange(n), per_pair)
    c = np.zeros(total, dtype=capi.PAIR_CANDIDATE_DT)
    top = rng.integers(100, 156, (n, 2))
    c["score"] = top[pair_of] - rng.integers(0, 12, (total, 2))
    c["distance"] = np.rint(400 + 40 * rng.normal(0, 1, total)).astype(np.int64)
    c["distance"][rng.random(total) < 0.05] = capi.INT64_MAX
    c["aln"] = rng.integers(0, 3, (total, 2)); c["better_cluster_count"] = rng.choice([1, 1, 1, 2, 3], total); c["aligned"] = 3
    kind = rng.random(n)                                              # 85 % of the pairs paired, the rest rescued from either mate
    c["type"] = np.where(kind[pair_of] < 0.85, 0, rng.integers(2, 4, total))
    counts = np.zeros(n, dtype=capi.PAIR_COUNTS_DT); counts["unpaired_count"] = rng.integers(0, 6, (n, 2)); counts["rescued_count"] = rng.integers(1, 6, (n, 2))
    reads = workloads.ACGT[rng.integers(0, 4, 2 * n * LENGTH)]
    read_off = np.arange(2 * n + 1, dtype=np.uint64) * np.uint64(LENGTH)
    quality = rng.integers(20, 42, 2 * n * LENGTH).astype(np.uint8)
    quality[rng.random(2 * n * LENGTH) < 0.02] = 8
    small = workloads.GaplessWorkload(10, seed=1, graph_bp=20000)
    eng = capi.Engine(lib=os.path.join(ROOT, "vg_amd", "libvgamd.so"), device=0)
    mindex = eng.minimizer_index(small.nodes, small.threads, k=K, w=W)
    moff, recs = eng.minimizer_list(mindex, reads, read_off)
    regions = eng.minimizer_regions(K, W, read_off, moff, recs)
    explored = (rng.random(len(recs)) < 0.7).astype(np.uint8)
    scheme = capi.PairMapqScheme(1.3833252687386448, 400.0, 40.0, 1, 15, K, 0)
    base = dict(cand_off=cand_off, candidates=c, counts=counts)
    sweep = dict(base, minimizer_off=moff, minimizers=recs, regions=regions, explored=explored, read_off=read_off, quality=quality)
    h = pipeline._host_lib()
    shim = lambda a: capi.pair_mapq_call(h.vgh_pair_mapq, (), scheme, tail=(ctypes.c_int(THREADS),), **a)

    computed_ms, (got, got_score, got_order) = timed(5, lambda: eng.pair_mapq(scheme, **sweep))
    computed_kernels, launches, computed_launches = eng.pair_mapq_last_ms(), eng.pair_mapq_last_launches(), eng.pair_mapq_last_kernel_launches()
    given = dict(base, given_cap=got["explored_cap"].ravel().copy())
    given_ms, (got2, _, _) = timed(5, lambda: eng.pair_mapq(scheme, **given))
    given_kernels, given_launches = eng.pair_mapq_last_ms(), eng.pair_mapq_last_kernel_launches()
    shim_computed_ms, (rc, want, want_score, want_order) = timed(2, lambda: shim(sweep), warm=0)
    shim_given_ms, (rc2, want2, _, _) = timed(2, lambda: shim(given), warm=0)
    assert rc == 0 and rc2 == 0 and (got["status"] == want["status"]).all() and got_score.tobytes() == want_score.tobytes() and (got_order == want_order).all()
    assert got2["mapq"].tobytes() == got["mapq"].tobytes()
    out = {"section": section, "pairs": n, "candidates": total, "read_length": LENGTH, "minimizers": int(len(recs)), "explored": int(explored.sum()), "host_threads": THREADS,
           "caps_in_the_call_ms": {"engine_call": computed_ms, "sweep_kernels": round(computed_kernels[0], 2), "pair_kernels": round(computed_kernels[1], 2), "shim_min": shim_computed_ms["min"]},
           "given_caps_ms": {"engine_call": given_ms, "pair_kernels": round(given_kernels[1], 2), "shim_min": shim_given_ms["min"]},
           "kernel_launches": {"caps_in_the_call": sum(computed_launches), "given_caps": sum(given_launches)}, "pairs_by_launch": {"lds": launches[0], "slab": launches[1], "refused": launches[2]},
           "mapq_differs_from_shim": int((got["mapq"] != want["mapq"]).any(axis=1).sum()), "mapq_differs_by_more_than_1": int((np.abs(got["mapq"] - want["mapq"]) > 1).any(axis=1).sum()),
           "mapq_histogram": {"0": int((got["mapq"] == 0).sum()), "1-59": int(((got["mapq"] > 0) & (got["mapq"] < 60)).sum()), "60": int((got["mapq"] == 60).sum())}}
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 3:
        with open(sys.argv[3], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
