#!/usr/bin/env python
"""What a read's mapping quality costs: vgk_minimizer_regions + vgk_read_mapq on the device against the host shim on 16 threads (profiles/r10_read_mapq).

    python tools/read_mapq_time.py short [reads [out.json]]     a million configs[2]-shaped reads (150 bp, k = 29, w = 11) with qualities
    python tools/read_mapq_time.py long [reads [out.json]]      4 000 reads of 15 kbp

One section per process, so that a job can run each under its own time limit.  The reads are random bases (what is timed reads no graph): their
minimizers are listed on the device (vgk_minimizer_list over a small index), 70 % of them explored, two scores per read, Illumina-like qualities.  The
engine's calls are timed host-inclusive (uploads, kernels, the way back; best of three), vgk_read_mapq_last_ms gives the kernels' share; the shim's
vgh_minimizer_regions and vgh_read_mapq run on 16 threads.  Prints one JSON line, and writes it to out.json when that is given."""
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vg_amd import capi, pipeline, workloads      # noqa: E402

K, W, THREADS = 29, 11, 16


def best_of(n, call):
    times = []
    for _ in range(n):
        t = time.perf_counter(); out = call(); times.append(time.perf_counter() - t)
    return min(times) * 1e3, out


def main():
    section = sys.argv[1] if len(sys.argv) > 1 else "short"
    n, length = {"short": (1_000_000, 150), "long": (4000, 15000)}[section]
    if len(sys.argv) > 2:
        n = int(sys.argv[2])
    rng = np.random.default_rng(10)
    reads = workloads.ACGT[rng.integers(0, 4, n * length)]
    read_off = (np.arange(n + 1, dtype=np.uint64) * np.uint64(length))
    quality = rng.integers(20, 42, n * length).astype(np.uint8)
    quality[rng.random(n * length) < 0.02] = 8
    small = workloads.GaplessWorkload(10, seed=1, graph_bp=20000)
    eng = capi.Engine(lib=os.path.join(ROOT, "vg_amd", "libvgamd.so"), device=0)
    mindex = eng.minimizer_index(small.nodes, small.threads, k=K, w=W)
    moff, recs = eng.minimizer_list(mindex, reads, read_off)
    explored = (rng.random(len(recs)) < 0.7).astype(np.uint8)
    top = rng.integers(length // 2, length + 6, n)
    scores = np.stack([top, top - rng.integers(0, 25, n)], axis=1).astype(np.int32).ravel()
    score_off = np.arange(n + 1, dtype=np.uint64) * np.uint64(2)
    scheme = capi.ReadMapqScheme(1.3833252687386448, 1.0, 0, K, 0, 0)
    h = pipeline._host_lib()

    regions_ms, regions = best_of(3, lambda: eng.minimizer_regions(K, W, read_off, moff, recs))
    regions_kernel_ms = eng.read_mapq_last_ms()[0]
    shim_regions_ms, (rc, shim_regions) = best_of(1, lambda: capi.minimizer_regions_call(h.vgh_minimizer_regions, (), K, W, read_off, moff, recs,
                                                                                         between=(ctypes.c_void_p(reads.ctypes.data),), tail=(ctypes.c_int(THREADS),)))
    assert rc == 0 and (regions == shim_regions).all()
    a = dict(score_off=score_off, scores=scores, minimizer_off=moff, minimizers=recs, regions=regions, explored=explored, read_off=read_off, quality=quality)
    mapq_ms, got = best_of(3, lambda: eng.read_mapq(scheme, **a))
    mapq_kernel_ms = eng.read_mapq_last_ms()[1]
    launches = eng.read_mapq_last_launches()
    shim_mapq_ms, (rc, want) = best_of(1, lambda: capi.read_mapq_call(h.vgh_read_mapq, (), scheme, tail=(ctypes.c_int(THREADS),), **a))
    assert rc == 0 and (got["status"] == want["status"]).all()
    out = {"section": section, "reads": n, "read_length": length, "minimizers": int(len(recs)), "explored": int(explored.sum()), "host_threads": THREADS,
           "regions_ms": {"engine_call": round(regions_ms, 2), "engine_kernel": round(regions_kernel_ms, 3), "shim": round(shim_regions_ms, 1)},
           "mapq_ms": {"engine_call": round(mapq_ms, 2), "engine_kernels": round(mapq_kernel_ms, 2), "shim": round(shim_mapq_ms, 1)},
           "reads_by_launch": {"lds": launches[0], "slab": launches[1], "refused": launches[2]},
           "mapq_differs_from_shim": int((got["mapq"] != want["mapq"]).sum()), "mapq_differs_by_more_than_1": int((np.abs(got["mapq"] - want["mapq"]) > 1).sum()),
           "cap_max_relative_error": float(np.nanmax(np.where(np.isfinite(want["explored_cap"]) & (want["explored_cap"] != 0),
                                                              np.abs(got["explored_cap"] - want["explored_cap"]) / np.abs(np.where(want["explored_cap"] == 0, 1, want["explored_cap"])), 0.0))),
           "mapq_histogram": {"0": int((got["mapq"] == 0).sum()), "1-59": int(((got["mapq"] > 0) & (got["mapq"] < 60)).sum()), "60": int((got["mapq"] == 60).sum())}}
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 3:
        with open(sys.argv[3], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
