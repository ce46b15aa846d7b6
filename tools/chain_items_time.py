#!/usr/bin/env python3
"""One batch of chaining problems shaped like the long-read stage's: 8 000 (read, tree) problems of 15 kbp reads, a 3 000-base graph lookback, anchor
counts taken from what vgk_minimizer_find_seeds yields for such reads under GIRAFFE_LONG_READ_POLICY (taken minimizers -> planted anchors, the other
seeds -> decoys).  Prints one JSON line: the three kernel times and the wall time of vgk_chain_items, and — labelled as what it is, the CHECKER, not a
baseline — the host shim's find_best_chains on 16 host threads for the same batch.
    python tools/chain_items_time.py [--problems 8000] [--distinct 250] [--sample 48]"""
import argparse, ctypes, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vg_amd import capi, pipeline, workloads

ap = argparse.ArgumentParser()
ap.add_argument("--problems", type=int, default=8000); ap.add_argument("--distinct", type=int, default=250); ap.add_argument("--sample", type=int, default=48)
args = ap.parse_args()
L = 15000; K = 29
eng = capi.Engine(capi.Scoring.simple(1, 4, 6, 1, 5))
# ---- what find_seeds yields for 15 kbp reads
g = workloads.VariationGraph(ref_len=4_000_000)
rng = np.random.default_rng(7)
comp = workloads._comp_table()
reads = np.empty((args.sample, L), dtype=np.uint8)
for i in range(args.sample):
    hseq = g.haps[int(rng.integers(0, 2))][0]; a = int(rng.integers(0, len(hseq) - L)); r = hseq[a:a + L]
    reads[i] = comp[r[::-1]] if rng.random() < 0.5 else r
sub = rng.random(reads.shape) < 0.005
reads[sub] = workloads.ACGT[rng.integers(0, 4, int(sub.sum()))]
off = np.arange(args.sample + 1, dtype=np.uint64) * L
threads = [(2 * np.nonzero(hap_pos >= 0)[0]).astype(np.uint32) for _, hap_pos in g.haps]
mi = eng.minimizer_index((g.node_len, g.seq), threads)
moff, recs, take, soff, seeds = eng.minimizer_find_seeds(mi, pipeline.GIRAFFE_LONG_READ_POLICY, reads.ravel(), off)
taken = int(round(float(take.sum()) / args.sample)); per_read = int(round(len(seeds) / args.sample))
n_planted = max(1, min(taken, L // (K + 3) - 1)); n_decoys = max(0, per_read - n_planted)
# ---- the batch: `distinct` problems made, repeated up to `problems`
wl = workloads.ChainItemsWorkload(min(args.distinct, args.problems), seed=3, read_len=L, n_planted=n_planted, n_decoys=n_decoys, graph_lookback=3000, seed_length=K, min_len=K, max_len=K)
problems = [wl.problems[i % len(wl.problems)] for i in range(args.problems)]
aoff, anchors, coff, cands = pipeline.pack_chain_problems(problems)
S = dict(max_chains=4, max_indel_bases=2000)
wall = []; dev = []
for rep in range(4):
    t = time.perf_counter(); out = eng.chain_items(S, aoff, anchors, coff, cands); wall.append(time.perf_counter() - t); dev.append(eng.chain_items_last_ms())
t = time.perf_counter()
rc, ref = capi.chain_items_call(pipeline._host_lib().vgh_find_best_chains, (), S, aoff, anchors, coff, cands, tail=(ctypes.c_void_p(None), ctypes.c_int(16)))
shim_s = time.perf_counter() - t
first = [out["items"][int(c["item_begin"]):int(c["item_begin"]) + int(c["n_items"])].tolist() for c in out["chains"][out["chain_off"][:-1].astype(np.int64)][:len(wl.problems)]]
print(json.dumps(dict(problems=args.problems, distinct=len(wl.problems), anchors_per_problem=n_planted + n_decoys, planted=n_planted, seeds_per_read=per_read, taken_per_read=taken,
                      candidates=int(len(cands)), kernel_ms=dict(legality_grouping=dev[-1][0], dp=dev[-1][1], traceback=dev[-1][2]), kernel_ms_all=dev,
                      call_wall_s_median_warm=float(np.median(wall[1:])), call_wall_s_all=wall, checker_shim_16_threads_s=shim_s,
                      identical_to_checker=bool(rc == 0 and all(out[f].tobytes() == ref[f].tobytes() for f in ("chain_off", "chains", "items", "table_score", "table_source"))),
                      planted_found=int(sum(x == t for x, t in zip(first, wl.truth))))))
