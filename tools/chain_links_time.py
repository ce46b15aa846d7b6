#!/usr/bin/env python
"""What a chain's links cost: vgk_chain_links on the device against the host shim on 16 threads (profiles/r13_chain_links).

    python tools/chain_links_time.py [out.json [scale]]     scale divides every shape's chain count (a quick look: 8)

Shapes, one chain per read and per anchor set, giraffe's hifi preset, a fifth of the anchors repetitive in runs of at most two, distances given from every
anchor to its next three (what the skip loop and a taken skip ask for), a twentieth of them off by 60 - 200 bases:
    4 000 and 32 000 chains of 15 kbp reads with about 57 anchors of 29 bases (LongReadWorkload's shape)
    the same reads with about 500 anchors of 15 bases (what find_seeds leaves for a long read)
    100 000 chains of 8 anchors on reads of about 300 bases
The reads are random bases (what is timed reads no graph).  The engine's call is timed host-inclusive (checks, uploads from pageable memory, kernels, the
way back; best of three after a warm-up, at the bounds the header names: no sizing call), vgk_chain_links_last_ms gives the kernels' share; the shim runs
once on 16 threads over the same inputs and must give the same answer, every field and byte.  Prints one JSON line, and writes it to out.json when given."""
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vg_amd import capi, pipeline, workloads      # noqa: E402

THREADS = 16


def best_of(n, call):
    times = []
    for _ in range(n):
        t = time.perf_counter(); out = call(); times.append(time.perf_counter() - t)
    return min(times) * 1e3, out


def shape(rng, n, m, length, gap_lo, gap_hi):
    """n chains of m anchors of `length` bases, gaps uniform in [gap_lo, gap_hi]"""
    gaps = rng.integers(gap_lo, gap_hi + 1, (n, m))
    start = gaps.cumsum(axis=1) + length * np.arange(m)[None, :]
    read_len = start[:, -1] + length + rng.integers(0, 100, n)
    anchors = np.zeros(n * m, dtype=capi.CHAIN_ANCHOR_DT)
    anchors["read_start"] = start.ravel(); anchors["length"] = length
    sites = np.zeros(n * m, dtype=capi.CHAIN_SITE_DT)
    sites["start_node"] = rng.integers(0, 1 << 20, n * m); sites["end_node"] = sites["start_node"] + rng.integers(0, 2, n * m) * 2
    sites["start_offset"] = rng.integers(0, 32, n * m); sites["end_offset"] = rng.integers(1, 33, n * m); sites["flags"] = (rng.random(n * m) < 0.3) & (np.tile(np.arange(m), n) % 3 != 0)      # (runs of at most two repetitive anchors: a skip reaches here + 3 at most)
    read_off = np.concatenate([[0], np.cumsum(read_len)]).astype(np.uint64)
    reads = workloads.ACGT[rng.integers(0, 4, int(read_off[-1]))]
    # per chain, ascending by (from, to): every anchor to its next three
    pairs = [(i, j) for i in range(m) for j in range(i + 1, min(m, i + 4))]
    frm = np.array([i for i, _ in pairs]); to = np.array([j for _, j in pairs])
    true = start[:, to] - (start[:, frm] + length)
    off = np.where(rng.random(true.shape) < 0.05, rng.integers(60, 200, true.shape), 0)
    dist = np.zeros(n * len(frm), dtype=capi.CHAIN_CANDIDATE_DT)
    dist["from"] = np.tile(frm, n); dist["to"] = np.tile(to, n); dist["graph_distance"] = (true + off).ravel()
    chains = np.zeros(n, dtype=capi.CHAIN_PROBLEM_DT)
    chains["read"] = chains["anchor_set"] = np.arange(n); chains["item_begin"] = np.arange(n) * m; chains["n_items"] = m
    return (reads, read_off, np.arange(n + 1, dtype=np.uint64) * np.uint64(m), anchors, sites, np.tile(np.arange(m, dtype=np.uint32), n),
            np.arange(n + 1, dtype=np.uint64) * np.uint64(len(frm)), dist, chains)


def main():
    scale = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    rng = np.random.default_rng(13)
    eng = capi.Engine(capi.Scoring.simple(1, 4, 6, 1, 5), lib=os.path.join(ROOT, "vg_amd", "libvgamd.so"), device=0)
    scheme = capi.ChainLinksScheme.hifi()
    h = pipeline._host_lib()
    rows = []
    for name, n, m, length, lo, hi in (("4 000 chains, 15 kbp, 57 anchors", 4000, 57, 29, 120, 350), ("32 000 chains, 15 kbp, 57 anchors", 32000, 57, 29, 120, 350),
                                       ("4 000 chains, 15 kbp, 500 anchors", 4000, 500, 15, 5, 25), ("32 000 chains, 15 kbp, 500 anchors", 32000, 500, 15, 5, 25),
                                       ("100 000 chains, 300 bp, 8 anchors", 100000, 8, 20, 5, 30)):
        n = max(1, n // scale)
        a = shape(rng, n, m, length, lo, hi)
        eng.chain_links(scheme, *a)                                                       # warm-up: the scratch slots are allocated
        ms, (rc, got) = best_of(3, lambda: eng.chain_links(scheme, *a))
        kernels = eng.chain_links_last_ms()
        shim, (rc2, want) = best_of(1, lambda: capi.chain_links_call(h.vgh_chain_links, (), scheme, *a, tail=(ctypes.c_int(THREADS),)))
        assert rc == 0 and rc2 == 0 and got["written"] == want["written"]
        assert all(got[k].tobytes() == want[k].tobytes() for k in ("results", "links", "kept", "seq_off", "seqs"))
        res = got["results"]
        rows.append({"shape": name, "chains": n, "anchors": n * m, "read_bases": int(a[1][-1]), "links": got["written"][0], "kept": got["written"][1], "seq_bytes": got["written"][2],
                     "cut": int((res["flags"] & capi.CHAIN_LINKS_CUT != 0).sum()), "dp_links": int((got["links"]["route"] == capi.CHAIN_ROUTE_DP).sum()),
                     "engine_call_ms": round(ms, 2), "kernels_ms": {"walk": round(kernels[0], 3), "scan_write": round(kernels[1], 3), "sequences": round(kernels[2], 3)},
                     "shim_ms": round(shim, 1)})
        del a, got, want
    out = {"host_threads": THREADS, "engine_calls_timed": 3, "shim_calls_timed": 1, "scale": scale, "shapes": rows, "answers_equal_the_shim_s": True}
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
