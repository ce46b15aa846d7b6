"""The offset form of the speculative first fill's rows (gssw_device.hpp: gssw_row_offset, lane_row).

Every H / E / F of that fill is carried as value + A in both halves of a register, A = the largest of the (scaled) gap open, gap extension and
profile bias.  Then none of a row's four subtractions can borrow from the other read's half — they are full-width subtracts instead of saturating
packed ones —, the zero floor is the third input of the E and F maxima, and H needs none.  The results must be what they were.

Every batch here (1 024 reads or a few more: the smallest that speculate) runs on the engine's own lane code in the CPU emulator and, under
`@pytest.mark.gpu`, on the HIP engine: every field and every op against the oracle, and against the same library with the form switched off when the
batch is packed (VGAMD_NO_OFFSET_ROWS=1).  Batch.row_offset() says that the form was really on (and off), so that a form quietly switched off
cannot pass.  The emulator is built with VGK_PK_CHECK: every full-width add / subtract of packed halves counts the calls that carry or borrow
(vgk_pk_check_failures) — none may, which is the proof obligation of the form.

The C ABI carries gap penalties in 8 bits, so the largest constant a caller can ask for is 8 * 255 = 2 040, far inside what the form admits
(8 * 990 + A + 255 < 0x7c00): a gap open "outside" cannot be packed, and the largest one stands for the edge."""
import ctypes
import subprocess

import numpy as np
import pytest

from test_refill_bound import BASES, LOCAL_TB, chain, linear_problem, rand_seq, same
from util import EMU_LIB, ENGINE_LIB, ORACLE_LIB, ROOT
from vg_amd import capi

N_READS = 1040
SCALE = 8


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.check_call(["make", "-s", "emu"], cwd=ROOT)
    return EMU_LIB


@pytest.fixture(params=["emu", pytest.param("hip", marks=pytest.mark.gpu)])
def lib(request):
    return request.getfixturevalue("emu_lib") if request.param == "emu" else ENGINE_LIB


def pk_failures(lib):
    if lib != EMU_LIB:
        return 0
    f = ctypes.CDLL(lib).vgk_pk_check_failures
    f.restype = ctypes.c_uint64
    return int(f())


def window(rng, width=None):
    width = int(rng.choice([384, 416])) if width is None else width
    return rand_seq(rng, width)


def problem(read, ref):
    nodes, preds = chain(ref)
    return {"read": read, "nodes": nodes, "preds": preds, "flags": LOCAL_TB, "pinning": None}


def headline(rng):
    return [linear_problem(rng, 0.001) for _ in range(N_READS)]


def mixed_lengths(rng):
    """reads of 145 - 150 bases in one batch — the lengths that share the 150-base reads' geometry (19 rows x 8 lanes; a batch of two geometries
    does not speculate): between 2 and 7 of the last lane's rows are padding rows (profile word 0: they score -bias against every base)"""
    return [linear_problem(rng, 0.001, read_len=int(rng.integers(145, 151))) for _ in range(N_READS)]


def floor_reads(rng):
    """reads that share no base with their window (every cell at the floor, score 0), reads of all N, and ordinary reads between them"""
    out = []
    for k in range(N_READS):
        if k % 3 == 0:
            out.append(linear_problem(rng, 0.001))
        elif k % 3 == 1:
            b = BASES[int(rng.integers(0, 4))]
            ref = "".join(c if c != b else BASES[(BASES.index(b) + 1) % 4] for c in window(rng))
            out.append(problem(b * 150, ref))
        else:
            out.append(problem("N" * 150, window(rng)))
    return out


def n_columns(rng):
    """windows with N columns, single ones and runs, inside and outside the read's span (the rows' REFN branch)"""
    out = []
    for _ in range(N_READS):
        p = linear_problem(rng, 0.001)
        ref = list("".join(p["nodes"]))
        for _ in range(int(rng.integers(1, 6))):
            at = int(rng.integers(0, len(ref) - 4)); ln = int(rng.integers(1, 4))
            ref[at:at + ln] = "N" * ln
        out.append(problem(p["read"], "".join(ref)))
    return out


def snp_bubbles(rng):
    """a SNP bubble of two one-base nodes in every window: last columns go to the scratch and come back as seeds (store_to_scratch /
    seed_from_scratch convert between the two forms), and the diagonal walk reads several predecessors"""
    out = []
    for _ in range(N_READS):
        p = linear_problem(rng, 0.01)
        nodes, v = p["nodes"], int(rng.integers(2, 9))
        a, alt = nodes[v][15], BASES[(BASES.index(nodes[v][15]) + 1) % 4]
        nodes = nodes[:v] + [nodes[v][:15], a, alt, nodes[v][16:]] + nodes[v + 1:]
        preds = [[]] + [[k - 1] for k in range(1, len(nodes))]
        preds[v + 2] = [v]; preds[v + 3] = [v + 1, v + 2]
        out.append(dict(p, nodes=nodes, preds=preds))
    return out


BATCHES = {"headline": (headline, 1), "mixed lengths": (mixed_lengths, 2), "floor reads": (floor_reads, 3), "N columns": (n_columns, 4),
           "SNP bubbles": (snp_bubbles, 5)}
_made = {}


def batch(name, sc):
    """-> (ProblemSet, the oracle's results and ops): made once, shared by the emulator's and the device's tests, never written"""
    key = (name, bytes(sc))
    if key not in _made:
        if name not in _made:
            make, seed = BATCHES[name]
            _made[name] = capi.ProblemSet.from_lists(make(np.random.default_rng(800 + seed)))
        ps = _made[name]
        _made[key] = (ps,) + tuple(capi.Engine(sc, lib=ORACLE_LIB).align(ps, 0))
    return _made[key]


def run(lib, ps, sc, monkeypatch, form, orders=(1,)):
    """one resident batch, packed with the form on or off, run once per entry of `orders` (1 = speculate, 2 = plain) -> ([(results, ops)], row offset)"""
    if not form:
        monkeypatch.setenv("VGAMD_NO_OFFSET_ROWS", "1")
    try:
        eng = capi.Engine(sc, lib=lib)
        out = []
        with eng.pack(ps, 0) as b:
            off = b.row_offset()
            for mode in orders:
                eng.set_speculation(mode)
                b.run(); b.sync()
                assert b.speculated() == (mode == 1)
                r, o = b.fetch()
                out.append((r.copy(), o.copy()))
        return out, off
    finally:
        if not form:
            monkeypatch.delenv("VGAMD_NO_OFFSET_ROWS")


def expected_offset(sc):
    mismatch = max(0, -min(sc.matrix))
    return SCALE * max(sc.gap_open, sc.gap_extend, mismatch)


def check(lib, monkeypatch, name, sc, orders=(1,)):
    ps, ro, oo = batch(name, sc)
    before = pk_failures(lib)
    on, off_on = run(lib, ps, sc, monkeypatch, True, orders)
    off, off_off = run(lib, ps, sc, monkeypatch, False, orders)
    assert off_on == expected_offset(sc) > 0 and off_off == 0, (name, off_on, off_off)
    for k, ((r, o), (r2, o2)) in enumerate(zip(on, off)):
        same(r, o, ro, oo, (name, "offset rows", k)); same(r2, o2, ro, oo, (name, "switched off", k))
    assert pk_failures(lib) == before, (name, "a full-width add or subtract carried or borrowed across the halves")
    return ro


DEFAULT = (1, 4, 6, 1, 5)


@pytest.mark.parametrize("name", list(BATCHES))
def test_offset_rows_match_the_oracle_and_the_saturating_rows(lib, monkeypatch, name):
    ro = check(lib, monkeypatch, name, capi.Scoring.simple(*DEFAULT))
    if name == "floor reads":
        # (a bonus on the first and the last read base can outweigh a mismatch or meet an N: scores up to the two bonuses; exactly 0 in test_scorings)
        assert (ro["score"][1::3] <= 2 * DEFAULT[4]).all() and (ro["score"][2::3] <= 2 * DEFAULT[4]).all() and (ro["score"][0::3] > 100).all()
    else:
        assert (ro["score"] > 60).mean() > 0.95


@pytest.mark.parametrize("scores", [(1, 4, 6, 1, 0),        # no full-length bonus
                                    (6, 4, 6, 1, 5),        # a match worth 6: 150 * 6 + 10 = 910 of the 990 the three-input key maximum admits
                                    (1, 4, 255, 1, 5),      # the largest gap open the ABI carries: A = 2 040
                                    (1, 4, 7, 1, 5),        # A = 8 * 7: the gap open decides, just above the bias ...
                                    (1, 7, 6, 1, 5),        # ... and the bias does, just above the gap open
                                    (1, 4, 2, 3, 5),        # ge > go
                                    (1, 2, 1, 9, 5)])       # the gap extension decides
def test_scorings(lib, monkeypatch, scores):
    check(lib, monkeypatch, "headline", capi.Scoring.simple(*scores))
    if scores[4] == 0:                                     # without a bonus the reads that share no base with their window, and the reads of N, score exactly 0
        ro = check(lib, monkeypatch, "floor reads", capi.Scoring.simple(*scores))
        assert (ro["score"][1::3] == 0).all() and (ro["score"][2::3] == 0).all()
    if scores[0] == 6:
        check(lib, monkeypatch, "SNP bubbles", capi.Scoring.simple(*scores))


def test_speculative_plain_speculative_on_one_resident_batch(lib, monkeypatch):
    check(lib, monkeypatch, "SNP bubbles", capi.Scoring.simple(*DEFAULT), orders=(1, 2, 1))


def test_no_call_of_this_process_carried_or_borrowed(emu_lib):
    """the counter is never reset: whatever ran on the emulator in this process before — other modules' batches included — is held to it as well"""
    assert pk_failures(emu_lib) == 0
