#!/usr/bin/env python
"""What choosing a long read's mappings costs: vgk_pick_mappings on the device against the host shim on 16 threads (profiles/r14_pick_mappings).

    python tools/pick_mappings_time.py [out.json [scale]]     scale divides every shape's read count (a quick look: 8)

Shapes — every read with as many chains as alignments, a tenth of the chains in a second component, ranges of 100 .. 300 bases from a 600-base stretch;
an alignment's mappings on nodes drawn from a pool of twice its read's mean mapping count (so later alignments share about half their nodes with the
first), 1.23 edit runs per mapping; scores 1000 less 40 per alignment; a generator per read:
    32 000 reads x 1 alignment x ~500 mappings                 the defaults (max_multimaps 1, fraction 0)
    32 000 reads x 4 alignments x ~500 mappings                the defaults
    4 000 reads x 16 alignments x ~500 mappings                max_multimaps 3, fraction 0.5: the used set of three alignments does not fit LDS
    1 000 000 reads x 2 alignments x 3 mappings                the defaults
The engine's call is timed host-inclusive (checks, uploads from pageable memory, kernels, the way back; best of three after a warm-up),
vgk_pick_mappings_last_ms gives the kernels' share; the shim runs once on 16 threads over the same inputs and must give the same answer, every field and
bit.  Prints one JSON line, and writes it to out.json when given."""
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


def shape(rng, n, A, lo, hi):
    """n reads of A alignments of lo .. hi mappings"""
    chains = np.zeros(n * A, dtype=capi.PICK_CHAIN_DT)
    chains["score_estimate"] = np.tile(900 - 30 * np.arange(A), n); chains["multiplicity"] = 1.0
    chains["range"]["component"] = rng.random(n * A) < 0.1
    start = rng.integers(0, 300, n * A); chains["range"]["offset_start"] = start; chains["range"]["offset_end"] = start + rng.integers(100, 300, n * A)
    count = rng.integers(lo, hi + 1, n * A).astype(np.int64)
    first = np.concatenate([[0], np.cumsum(count)])
    total = int(first[-1])
    alns = np.zeros(n * A, dtype=capi.PICK_ALIGNMENT_DT)
    alns["source"] = np.tile(np.arange(A), n); alns["score"] = np.tile(1000 - 40 * np.arange(A), n); alns["item_count"] = np.tile(np.arange(1, A + 1), n)
    alns["result"]["mapping_begin"] = first[:-1]; alns["result"]["n_mappings"] = count
    read_of = np.repeat(np.repeat(np.arange(n, dtype=np.int64), A), count)
    mappings = np.zeros(total, dtype=capi.CHAIN_MAPPING_DT)
    mappings["node"] = read_of * (2 * (lo + hi)) + rng.integers(0, lo + hi, total)
    second = rng.random(total) < 0.23
    mappings["n_edits"] = 1 + second
    begin = np.concatenate([[0], np.cumsum(mappings["n_edits"], dtype=np.int64)])
    mappings["edit_begin"] = begin[:-1]
    edits = np.full(int(begin[-1]), (30 << 2) | 0, dtype=np.uint32)
    edits[begin[:-1][second] + 1] = (1 << 2) | rng.integers(1, 4, int(second.sum()))
    read_off = np.arange(n + 1, dtype=np.uint64) * np.uint64(32)
    reads = workloads.ACGT[rng.integers(0, 4, 32 * n)]
    off = np.arange(n + 1, dtype=np.uint64) * np.uint64(A)
    return (reads, read_off, off, chains, off, alns, mappings, edits)


def main():
    scale = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    rng = np.random.default_rng(14)
    eng = capi.Engine(capi.Scoring.simple(1, 4, 6, 1, 5), lib=os.path.join(ROOT, "vg_amd", "libvgamd.so"), device=0)
    h = pipeline._host_lib()
    plain = capi.PickScheme.defaults(); three = capi.PickScheme.defaults(max_multimaps=3, min_unique_node_fraction=0.5)
    rows = []
    for name, scheme, n, A, lo, hi in (("32 000 reads x 1 alignment x ~500 mappings", plain, 32000, 1, 400, 600), ("32 000 reads x 4 alignments x ~500 mappings", plain, 32000, 4, 400, 600),
                                       ("4 000 reads x 16 alignments x ~500 mappings, three multimaps", three, 4000, 16, 400, 600),
                                       ("1 000 000 reads x 2 alignments x 3 mappings", plain, 1000000, 2, 3, 3)):
        n = max(1, n // scale)
        a = shape(rng, n, A, lo, hi)
        state = np.zeros(n, dtype=np.uint32)
        eng.pick_mappings(scheme, *a, rng_state=state.copy())                             # warm-up: the scratch slots are allocated
        ms, (rc, got) = best_of(3, lambda: eng.pick_mappings(scheme, *a, rng_state=state.copy()))
        kernels = eng.pick_mappings_last_ms(); launches = eng.pick_mappings_last_launches()
        shim, (rc2, want) = best_of(1, lambda: capi.pick_mappings_call(h.vgh_pick_mappings, (), scheme, *a, rng_state=state.copy(), tail=(ctypes.c_int(THREADS),)))
        assert rc == 0 and rc2 == 0 and got["written"] == want["written"]
        assert all(got[k].tobytes() == want[k].tobytes() for k in ("results", "verdicts", "picked", "scores", "multiplicity"))
        rows.append({"shape": name, "reads": n, "alignments": n * A, "mappings": len(a[6]), "edit_runs": len(a[7]), "max_multimaps": int(scheme.max_multimaps),
                     "min_unique_node_fraction": float(scheme.min_unique_node_fraction), "reads_lds_slab_refused": list(launches),
                     "reported": int(got["results"]["n_mappings"].sum()), "counted": int(got["results"]["n_scores"].sum()),
                     "failed_uniqueness": int((got["verdicts"]["fate"] == capi.PICK_FAIL_UNIQUE).sum()),
                     "engine_call_ms": round(ms, 2), "kernels_ms": {"checks": round(kernels[0], 3), "statistics": round(kernels[1], 3), "multiplicities": round(kernels[2], 3),
                                                                    "pick": round(kernels[3], 3)},
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
