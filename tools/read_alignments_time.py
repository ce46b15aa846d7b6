#!/usr/bin/env python3
"""One configs[2]-shaped batch of short reads through seeds' clusters -> vgk_gapless_extend -> vgk_tail_stage_aligned -> vgk_read_alignments.  Prints one
JSON line: the three kernel groups' device ms and the wall time of vgk_read_alignments over the downloaded sets and tails (warm calls: median and all),
the wall time of the vgk_tail_stage_aligned call that precedes it on the same batch with the bytes each call brings down, the wall time and kernel ms
of vgk_tail_stage_composed — the resident form, which replaces both calls — on the same batch, and — labelled as what it is,
the CHECKER — the host shim's vgh_read_alignments on 16 host threads for the same input.
    python tools/read_alignments_time.py [--reads 1000000] [--graph-bp 4000000]"""
import argparse, ctypes, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vg_amd import capi, pipeline, workloads

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=1_000_000); ap.add_argument("--graph-bp", type=int, default=4_000_000); ap.add_argument("--window-length", type=int, default=39)
args = ap.parse_args()
scoring = (1, 4, 6, 1, 5)
eng = capi.Engine(capi.Scoring.simple(*scoring))
wl = workloads.GaplessWorkload(args.reads, seed=10, graph_bp=args.graph_bp, inserted_reads=0.3)
index = eng.haplo_index(wl.nodes, wl.threads)
stage_wall = []
for rep in range(3):
    res, ext, nodes, mism = eng.gapless_extend(index, wl.gs)
    t = time.perf_counter()
    ext_total, read_score, tails, tail_ops, stats = eng.tail_stage_aligned(index, wl.gs.n, len(ext))
    stage_wall.append(time.perf_counter() - t)
res, ext, nodes, mism, tails, tail_ops = (np.array(a) for a in (res, ext, nodes, mism, tails, tail_ops))
wall, dev = [], []
for rep in range(5):
    t = time.perf_counter()
    out = eng.read_alignments(index, wl.gs.reads, wl.gs.read_off, res, ext, nodes, mism, tails, tail_ops, window_length=args.window_length)
    wall.append(time.perf_counter() - t); dev.append(eng.read_alignments_last_ms())
composed_wall, composed_dev = [], []
for rep in range(4):
    eng.gapless_extend(index, wl.gs)
    t = time.perf_counter()
    c_total, c_score, made, c_stats = eng.tail_stage_composed(index, wl.gs.n, len(ext), window_length=args.window_length, caps=out["written"])
    composed_wall.append(time.perf_counter() - t); composed_dev.append(eng.read_alignments_last_ms())
resident_identical = bool(all(made[f].tobytes() == out[f].tobytes() for f in ("aln_off", "alignments", "mappings", "edits")) and (c_score == read_score).all())
comp = bytes.maketrans(b"ACGT", b"TGCA")
oseq = []
for s in wl.nodes:
    b = s.encode(); oseq += [b, b.translate(comp)[::-1]]
olen = np.array([len(b) for b in oseq], dtype=np.uint32); oflat = np.frombuffer(b"".join(oseq), dtype=np.uint8)
sc = np.array(scoring, dtype=np.int32)
t = time.perf_counter()
rc, ref = capi.read_alignments_call(pipeline._host_lib().vgh_read_alignments, (ctypes.c_void_p(sc.ctypes.data), ctypes.c_void_p(olen.ctypes.data), ctypes.c_void_p(oflat.ctypes.data),
                                                                              ctypes.c_uint64(len(olen))), wl.gs.reads, wl.gs.read_off, res, ext, nodes, mism, tails, tail_ops,
                                    window_length=args.window_length, caps=out["written"], tail=(ctypes.c_int(16),))
shim_s = time.perf_counter() - t
aln = out["alignments"]
best = aln[aln["kind"] != capi.READ_ALN_SECOND]
print(json.dumps(dict(reads=args.reads, graph_bp=args.graph_bp, extensions=int(len(ext)), tails=int(len(tails)), tail_ops=int(len(tail_ops)),
                      alignments=int(len(aln)), mappings=int(len(out["mappings"])), edit_runs=int(len(out["edits"])), direct=int((aln["kind"] == capi.READ_ALN_DIRECT).sum()),
                      empty_second=int(((aln["kind"] == capi.READ_ALN_SECOND) & (aln["n_mappings"] == 0)).sum()), bad_status=int((aln["status"] != 0).sum()),
                      kernel_ms=dict(select=dev[-1][0], count_scan=dev[-1][1], emit=dev[-1][2]), kernel_ms_all=dev,
                      read_alignments_wall_s_median_warm=float(np.median(wall[1:])), read_alignments_wall_s_all=wall,
                      read_alignments_bytes_down=int(aln.nbytes + out["mappings"].nbytes + out["edits"].nbytes + 8 * (wl.gs.n + 1)),
                      tail_stage_aligned_wall_s_median_warm=float(np.median(stage_wall[1:])), tail_stage_aligned_wall_s_all=stage_wall,
                      tail_stage_aligned_bytes_down=int(tails.nbytes + tail_ops.nbytes + ext_total.nbytes + read_score.nbytes),
                      tail_stage_composed_wall_s_median_warm=float(np.median(composed_wall[1:])), tail_stage_composed_wall_s_all=composed_wall, tail_stage_composed_kernel_ms_all=composed_dev,
                      tail_stage_composed_bytes_down=int(aln.nbytes + out["mappings"].nbytes + out["edits"].nbytes + 8 * (wl.gs.n + 1) + ext_total.nbytes + read_score.nbytes),
                      resident_identical_to_explicit=resident_identical,
                      checker_shim_16_threads_s=shim_s, identical_to_checker=bool(rc == 0 and all(out[f].tobytes() == ref[f].tobytes() for f in ("aln_off", "alignments", "mappings", "edits"))),
                      best_equals_read_score=int((best["score"][np.unique(best["read"], return_index=True)[1]] == read_score).sum()))))
