#!/usr/bin/env python
"""What a short read's funnel costs: vgk_funnel_clusters, vgk_funnel_extension_sets and vgk_funnel_winners on the device against the host shim on 16
threads (profiles/r12_read_funnel).

    python tools/read_funnel_time.py [reads [out.json]]     a million configs[2]-shaped reads (150 bp, k = 29, w = 11) with 1 to 8 synthetic clusters each

The reads are random bases (what is timed reads no graph): their minimizers are listed on the device (vgk_minimizer_list over a small index); a cluster is
1 to 6 seeds of random minimizers of its read; every kept cluster gets a synthetic extension set of 1 to 3 extensions in read order, every aligned set two
alignments.  Giraffe's default policy; every read carries a generator.  The engine's calls are timed host-inclusive (checks, uploads, kernels, the way back;
best of three, at a capacity known beforehand: no sizing call), vgk_funnel_last_ms gives the kernels' share; the shim's vgh_funnel_* run on 16 threads over the same inputs and must give the same answers.
Prints one JSON line, and writes it to out.json when that is given."""
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


def best_of(n, call):
    times = []
    for _ in range(n):
        t = time.perf_counter(); out = call(); times.append(time.perf_counter() - t)
    return min(times) * 1e3, out


def ragged(counts):
    """offsets of lists of `counts` items, and for every item the list it is in"""
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    return off, np.repeat(np.arange(len(counts), dtype=np.int64), counts)


def same(a, b, keys):
    return all(a[k].tobytes() == b[k].tobytes() for k in keys)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    rng = np.random.default_rng(12)
    reads = workloads.ACGT[rng.integers(0, 4, n * LENGTH)]
    read_off = np.arange(n + 1, dtype=np.uint64) * np.uint64(LENGTH)
    small = workloads.GaplessWorkload(10, seed=1, graph_bp=20000)
    eng = capi.Engine(capi.Scoring.simple(1, 4, 6, 1, 5), lib=os.path.join(ROOT, "vg_amd", "libvgamd.so"), device=0)
    moff, recs = eng.minimizer_list(eng.minimizer_index(small.nodes, small.threads, k=K, w=W), reads, read_off)
    recs["hits"] = rng.integers(1, 40, len(recs))
    scores = pipeline.minimizer_scores(recs)
    per_read = np.diff(moff.astype(np.int64))
    cluster_off, read_of_cluster = ragged(np.where(per_read > 0, rng.integers(1, 9, n), 0))
    cluster_seed_off, cluster_of_seed = ragged(rng.integers(1, 7, len(read_of_cluster)))
    sources = (rng.random(len(cluster_of_seed)) * per_read[read_of_cluster[cluster_of_seed]]).astype(np.uint32)
    pol = capi.FunnelPolicy.giraffe(K)
    h = pipeline._host_lib(); t = (ctypes.c_int(THREADS),)
    zero = lambda: np.zeros(n, dtype=np.uint32)

    a1 = (reads, read_off, moff, recs, scores, cluster_off, cluster_seed_off, sources)
    ms1, (rc, got1) = best_of(3, lambda: eng.funnel_clusters(pol, *a1, rng_state=zero(), cap=len(read_of_cluster)))
    kernel1 = eng.funnel_last_ms()[0]; launches1 = eng.funnel_last_launches()
    state = zero(); eng.funnel_clusters(pol, *a1, rng_state=state, cap=len(read_of_cluster))
    shim1, (rc, want1) = best_of(1, lambda: capi.funnel_clusters_call(h.vgh_funnel_clusters, (), pol, *a1, rng_state=zero(), tail=t, cap=len(read_of_cluster)))
    assert rc == 0 and same(got1, want1, ("clusters", "status", "kept_off", "kept"))

    kept_off, kept = got1["kept_off"], got1["kept"]
    n_sets = len(kept)
    n_ext = rng.integers(1, 4, n_sets)
    begins = np.sort(rng.integers(0, LENGTH - 40, (n_sets, 3)), axis=1)
    used = np.arange(3)[None, :] < n_ext[:, None]
    ext = np.zeros(int(n_ext.sum()), dtype=capi.EXT_DT)
    ext["read_begin"] = begins[used]; ext["read_end"] = ext["read_begin"] + rng.integers(12, 40, len(ext)); ext["score"] = rng.integers(8, 40, len(ext))
    res = np.zeros(n_sets, dtype=capi.GAPLESS_RESULT_DT)
    res["n_ext"] = n_ext; res["ext_begin"] = np.concatenate([[0], np.cumsum(n_ext)])[:-1]
    a2 = (reads, read_off, kept_off, res, ext, kept_off, kept, cluster_seed_off, sources, moff)
    entering = state.copy()
    ms2, (rc, got2) = best_of(3, lambda: eng.funnel_extension_sets(pol, *a2, rng_state=entering.copy(), cap=n_sets))
    kernel2 = eng.funnel_last_ms()[1]; launches2 = eng.funnel_last_launches()
    eng.funnel_extension_sets(pol, *a2, rng_state=state, cap=n_sets)
    shim2, (rc, want2) = best_of(1, lambda: capi.funnel_extension_sets_call(h.vgh_funnel_extension_sets, (), pol, *a2, rng_state=entering.copy(),
                                                                            between=(ctypes.c_int(6), ctypes.c_int(1)), tail=t, cap=n_sets))
    assert rc == 0 and same(got2, want2, ("sets", "status", "aligned_off", "aligned", "explored"))

    aligned_off = got2["aligned_off"]; n_aligned = len(got2["aligned"])
    top = rng.integers(LENGTH // 2, LENGTH + 6, n_aligned)
    aln_score = np.stack([top, top - rng.integers(0, 40, n_aligned)], axis=1).astype(np.int32).ravel()
    a3 = (reads, read_off, aligned_off, np.arange(n_aligned + 1, dtype=np.uint64) * np.uint64(2), aln_score, np.full(len(aln_score), 3, dtype=np.uint32))
    entering = state.copy()
    ms3, (rc, got3) = best_of(3, lambda: eng.funnel_winners(pol, *a3, rng_state=entering.copy(), cap=len(aln_score) + n))
    kernel3 = eng.funnel_last_ms()[2]; launches3 = eng.funnel_last_launches()
    shim3, (rc, want3) = best_of(1, lambda: capi.funnel_winners_call(h.vgh_funnel_winners, (), pol, *a3, rng_state=entering.copy(), tail=t, cap=len(aln_score) + n))
    assert rc == 0 and same(got3, want3, ("score_off", "scores", "reported", "n_reported", "unmapped"))

    out = {"reads": n, "read_length": LENGTH, "minimizers": int(len(recs)), "clusters": int(len(read_of_cluster)), "seeds": int(len(sources)), "kept": int(n_sets),
           "aligned": int(n_aligned), "scores": int(len(got3["scores"])), "host_threads": THREADS, "engine_calls_timed": 3, "shim_calls_timed": 1,
           "clusters_ms": {"engine_call": round(ms1, 2), "engine_kernels": round(kernel1, 2), "shim": round(shim1, 1)},
           "sets_ms": {"engine_call": round(ms2, 2), "engine_kernels": round(kernel2, 2), "shim": round(shim2, 1)},
           "winners_ms": {"engine_call": round(ms3, 2), "engine_kernels": round(kernel3, 2), "shim": round(shim3, 1)},
           "reads_by_launch": {"clusters": launches1, "sets": launches2, "winners": launches3}, "answers_equal_the_shim_s": True}
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
