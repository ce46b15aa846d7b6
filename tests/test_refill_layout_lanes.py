"""The layout of a speculative batch's second fill: a lane per missed read, the chain test at pack time.

Whether a read's window is a chain — every node's only predecessor is the node before it, the first node has none — is decided when the batch is
packed and kept in the descriptor (gssw_device.hpp: PD_CHAIN), by the host packer (vgk_gssw_pack) and by the device packer (vgk_gssw_pack_windows)
alike; refill_col0 reads the bit and finds the nodes begun before its column by bisection.  The layout itself is one function per read slot of the
miss list and one per wavefront (refill_layout_read / refill_layout_wave); the kernel runs a lane per slot, the emulator their serial composition.

Everything here runs the engine's own lane code on the CPU emulator, speculation forced on, against the oracle field by field and op by op, with
both packers: chain windows (the bound must apply: refill_stats()['bounded'] > 0), windows with a SNP bubble (it must not: 0), and a batch with
reads of another mode mixed in — pinned reads through the host packer, X-drop reads through the device packer, which offers no pinned windows —
where only the local reads can be bounded.  No walk may ask for a code left of its read's start ('broken' == 0)."""
import subprocess

import numpy as np
import pytest

from test_refill_bound import BASES, linear_problem, same
from util import EMU_LIB, ORACLE_LIB, ROOT
from vg_amd import capi

SC = capi.Scoring.simple(1, 4, 6, 1, 5)
N = 1100                                                                   # (a batch speculates from 1 024 reads on)


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.check_call(["make", "-s", "emu"], cwd=ROOT)
    return EMU_LIB


def with_snp_bubble(rng, p):
    """node v of a chain becomes: its first 15 bases, a SNP bubble of two one-base nodes, the rest"""
    nodes, v = p["nodes"], int(rng.integers(2, 9))
    a, alt = nodes[v][15], BASES[(BASES.index(nodes[v][15]) + 1) % 4]
    nodes = nodes[:v] + [nodes[v][:15], a, alt, nodes[v][16:]] + nodes[v + 1:]
    preds = [[]] + [[k - 1] for k in range(1, len(nodes))]
    preds[v + 2] = [v]; preds[v + 3] = [v + 1, v + 2]
    return dict(p, nodes=nodes, preds=preds)


def windows_of(problems):
    """the problems' graphs side by side as ONE resident graph, each problem a window of it -> (graph arrays for Engine.graph, WindowSet)"""
    node_len, seq, pred_off, pred_idx, first, count, reads, read_off, flags, gaps, cols = [], [], [0], [], [], [], [], [0], [], [], []
    for p in problems:
        base = len(node_len)
        first.append(base); count.append(len(p["nodes"])); flags.append(p["flags"]); gaps.append(p.get("max_gap", 0))
        cols.append(sum(len(s) for s in p["nodes"]))
        for s, pr in zip(p["nodes"], p["preds"]):
            node_len.append(len(s)); seq.append(s)
            pred_idx.extend(base + q for q in pr); pred_off.append(len(pred_idx))
        reads.append(p["read"]); read_off.append(read_off[-1] + len(p["read"]))
    arrays = (np.array(node_len, np.uint32), np.frombuffer("".join(seq).encode(), np.uint8), np.array(pred_off, np.uint32), np.array(pred_idx, np.uint32))
    ws = capi.WindowSet(np.frombuffer("".join(reads).encode(), np.uint8), read_off, first, count, np.array(flags, np.uint32), max_gap=gaps, cols=cols)
    return arrays, ws


def run_batch(lib, problems, packer, orders=(1,), ops_per=0, sc=SC, eng=None):
    """one resident batch, packed by `packer` ('pack' | 'pack_windows'), run once per entry of `orders` (1 = speculate, 2 = plain)
    -> [(results, ops, refill_stats)]"""
    eng = eng or capi.Engine(sc, lib=lib)
    if packer == "pack":
        b = eng.pack(capi.ProblemSet.from_lists(problems), ops_per)
    else:
        arrays, ws = windows_of(problems)
        b = eng.pack_windows(eng.graph(*arrays), ws, ops_per)
    out = []
    with b:
        for mode in orders:
            eng.set_speculation(mode)
            b.run(); b.sync()
            assert b.speculated() == (mode == 1), (packer, mode)
            st = b.refill_stats()
            r, o = b.fetch()
            out.append((r.copy(), o.copy(), st))
    return out


def oracle_of(problems, sc=SC):
    return capi.Engine(sc, lib=ORACLE_LIB).align(capi.ProblemSet.from_lists(problems), 0)


def chain_batch(seed):
    rng = np.random.default_rng(seed)
    return [linear_problem(rng, 0.01) for _ in range(N)]                  # 384 / 416 columns, 150-base reads, 1 % indels


def bubble_batch(seed):
    rng = np.random.default_rng(seed)
    return [with_snp_bubble(rng, linear_problem(rng, 0.01)) for _ in range(N)]


def mixed_batch(seed, other):
    """every sixth read in another mode (`other`: 'pinned' | 'xdrop') -> (problems, how many of those)"""
    rng = np.random.default_rng(seed)
    problems = [linear_problem(rng, 0.01) for _ in range(N)]
    for k in range(0, N, 6):
        p = problems[k]
        if other == "pinned":
            problems[k] = dict(p, flags=capi.VGK_GSSW_PINNED | capi.VGK_GSSW_TRACEBACK, pinning=[0] * (len(p["nodes"]) - 1) + [1])
        else:
            problems[k] = dict(p, flags=capi.VGK_XDROP_PINNED | capi.VGK_GSSW_TRACEBACK, max_gap=16)
    return problems, len(range(0, N, 6))


@pytest.mark.parametrize("packer", ["pack", "pack_windows"])
def test_chain_windows_are_bounded(emu_lib, packer):
    problems = chain_batch(21)
    ro, oo = oracle_of(problems)
    (r, o, st), = run_batch(emu_lib, problems, packer)
    same(r, o, ro, oo, ("chains", packer))
    print(packer, st)
    assert st["broken"] == 0 and st["missed"] > 100 and st["bounded"] > 0.9 * st["missed"], st
    assert st["waves"] == (st["missed"] + 15) // 16 and st["steps"] / st["waves"] < 260, st      # (150-base reads: 16 to a wavefront; unbounded: close to 400 steps)


@pytest.mark.parametrize("packer", ["pack", "pack_windows"])
def test_bubble_windows_are_not(emu_lib, packer):
    problems = bubble_batch(22)
    ro, oo = oracle_of(problems)
    (r, o, st), = run_batch(emu_lib, problems, packer)
    same(r, o, ro, oo, ("bubbles", packer))
    assert st["broken"] == 0 and st["missed"] > 100 and st["bounded"] == 0, st


@pytest.mark.parametrize("packer,other", [("pack", "pinned"), ("pack_windows", "xdrop")])
def test_reads_of_another_mode_are_not(emu_lib, packer, other):
    problems, n_other = mixed_batch(23, other)
    ro, oo = oracle_of(problems)
    (r, o, st), = run_batch(emu_lib, problems, packer)
    same(r, o, ro, oo, ("mixed", packer))
    # (the first walk leaves every pinned and X-drop read to the second fill: none of them may start right of column 0)
    assert st["broken"] == 0 and st["bounded"] > 0 and st["missed"] - st["bounded"] >= n_other, (st, n_other)


def test_both_packers_give_the_same_layout(emu_lib):
    """the chain bit is the packer's: both must give every read the same start — the same wavefronts, steps and bounded reads — on a batch that
    mixes chains with bubble windows"""
    rng = np.random.default_rng(24)
    problems = [linear_problem(rng, 0.01) if k % 3 else with_snp_bubble(rng, linear_problem(rng, 0.01)) for k in range(N)]
    ro, oo = oracle_of(problems)
    stats = []
    for packer in ("pack", "pack_windows"):
        (r, o, st), = run_batch(emu_lib, problems, packer)
        same(r, o, ro, oo, ("chains and bubbles", packer))
        assert st["broken"] == 0 and 0 < st["bounded"] < st["missed"], st
        stats.append(st)
    assert stats[0] == stats[1], stats


@pytest.mark.parametrize("packer", ["pack", "pack_windows"])
def test_speculative_plain_speculative_on_one_resident_batch(emu_lib, packer):
    """the plain run finds every read back at column 0 in its own wavefront (refill_restore_one), the third run lays the same reads out again"""
    problems = chain_batch(25)
    ro, oo = oracle_of(problems)
    runs = run_batch(emu_lib, problems, packer, orders=(1, 2, 1))
    for k, (r, o, st) in enumerate(runs):
        same(r, o, ro, oo, ("spec, plain, spec", packer, k))
        assert st["broken"] == 0
    assert runs[1][2]["missed"] == 0 and runs[1][2]["bounded"] == 0
    assert runs[0][2] == runs[2][2] and runs[0][2]["bounded"] > 0, (runs[0][2], runs[2][2])
