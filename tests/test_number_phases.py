"""msj_number_values_device (csrc/numbers_kernel.hip) with a number's features at every phase of its device-only readers:
WindowRuns -- the lane path's 64 bytes in LDS from the number's 16-byte line on, memory behind them, the byte-by-byte chunk
at the end of the buffer -- and WaveRuns, the ballots over 64 bytes per step of the numbers flagged MSJ_SPAN_LONG; and with
the fallback list filled exactly.  tests/test_number_math.py holds the arithmetic against Python on the CPU through the
serial reader only; a wrong answer of the other two is a wrong value that nothing else would notice.

The corpus is tests/number_phases.py.  Every record is compared bit for bit with the host twin and with Python
(tests.test_number_math.expected) by tests/test_numbers._check_call; there are no tolerances.  test_corpus_on_cpu pins the
corpus -- the counts, the place of every feature, that the texts with and without a far digit differ in their bits -- before
any GPU sees it.
"""
import ctypes
from collections import Counter

import numpy as np
import pytest

from tests import number_phases as nph
from tests import test_number_math as tnm
from tests import test_numbers as tn

UINT64_MAX = tn.UINT64_MAX
LONG = 128   # MSJ_SPAN_LONG
PLACES = 16 * 4            # group A: start residues x window offsets
A_TEXTS = {"dot": 2, "e": 2, "esign": 4, "elast": 2, "x": 2, "firstnz": 2, "tie": 6, "tie0": 6}   # per place: signs x forms
C_PAIRED = ("tie_frac", "tie_int", "sticky")
SPAN_CALLS = [("spans", 0), ("pairs", 0), ("spans", 1), ("spans", 2), ("pairs", 1), ("pairs", 2)]


@pytest.fixture(scope="module")
def dev():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mojo_simdjson_amd.device import Stage1Device

    d = Stage1Device(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def twin():
    return tnm.load_twin()


# ---- where a case's feature stands ------------------------------------------------------------------------------------------

def _exponent_digits(t):
    e = t.index(b"e")
    return e + 1 + (t[e + 1:e + 2] in (b"+", b"-"))


def _digit_800(t):
    """position of the significant digit of index kExactDigits (counted from 0 at the first non-zero digit)"""
    seen, started = 0, False
    for p, ch in enumerate(t):
        if ch in b"-.":
            continue
        started = started or ch != 0x30
        if started:
            if seen == nph.EXACT_DIGITS:
                return p
            seen += 1
    raise AssertionError("fewer digits")


def run_and_feature(c):
    """-> (start of the run that the wave reader walks, position of the case's feature), in the text"""
    t, kind = c.text, c.kind[:-1] if c.kind.endswith("0") else c.kind
    neg, dot = t[:1] == b"-", t.find(b".")
    body = t[:t.index(b"e")] if b"e" in t else t
    if kind == "int_dot":
        return neg + 1, dot
    if kind == "frac_e":
        return dot + 1, t.index(b"e")
    if kind == "frac_end":
        return dot + 1, len(t)
    if kind == "frac_x":
        return dot + 1, t.index(b"x")
    if kind == "exp_nz":
        eb = _exponent_digits(t)
        return eb, len(t) - len(t[eb:].lstrip(b"0"))
    if kind == "exp_end":
        return _exponent_digits(t), len(t)
    if kind == "firstnz":
        return dot + 1, t.index(b"7")
    if kind == "tie_frac":
        return dot + 1, neg + 19 + 1 + len(body[neg + 20:]) - len(body[neg + 20:].lstrip(b"0"))
    if kind == "tie_int":
        return neg + 19, neg + 19 + len(body[neg + 19:]) - len(body[neg + 19:].lstrip(b"0"))
    if kind == "sticky":
        at = _digit_800(t)
        return at, at + len(body[at:]) - len(body[at:].lstrip(b"0"))
    raise AssertionError(kind)


def mult64_run(c):
    """length of the run of the mult64 case that is an exact multiple of 64: the reader's last step finds nothing"""
    t = c.text
    neg, dot = t[:1] == b"-", t.find(b".")
    if t[neg:neg + 2] == b"0." or t[neg:neg + 20] == nph.TIE19 + b".":   # zero_frac, tie_tail: the fraction, all zeros
        run = t[dot + 1:t.index(b"e")]
        assert run.strip(b"0") == b""
        return len(run)
    if t[_exponent_digits(t):].strip(b"0") == b"":                      # zero_exp: the exponent's digits, all zeros
        return len(t) - _exponent_digits(t)
    return dot - neg - 1                                                # int_run: the integer's digits behind the first


def check_a_case(c, start):
    (s, o), t = c.phase, c.text
    at = o - s
    assert start % 16 == s and (start - (start & ~15)) + at == o and 47 <= at < len(t) <= 90, c
    lead = t[t[:1] == b"-":at]
    if c.kind == "dot":
        assert t[at:at + 1] == b"." and lead.isdigit() and t[at + 1:].isdigit()
    elif c.kind == "e":
        assert t[at:at + 1] in (b"e", b"E") and lead.isdigit()
    elif c.kind == "esign":
        assert t[at:at + 1] in (b"+", b"-") and t[at - 1:at] == b"e" and t[at + 1:].isdigit()
    elif c.kind == "elast":
        assert len(t) == at + 1 and t[at - 3:at - 1] == b"e-" and t[at - 1:].isdigit()
    elif c.kind == "x":
        assert len(t) == at + 1 and t[at:] == b"x" and lead.replace(b".", b"").isdigit()
    elif c.kind == "firstnz":
        assert t[at:at + 1] == b"7" and lead.strip(b"0.") == b""
    else:
        assert t[at:at + 1] == (b"1" if c.kind == "tie" else b"0"), c
        tie = lead[:19] if lead.startswith(nph.TIE19) else lead[:16]
        assert tie in (nph.TIE16, nph.TIE19) and lead[len(tie):].strip(b"0.") == b"" and t[at + 1:].lstrip(b"e-0123456789") == b""


def twin_and_python(twin, lay):
    """The twin on every case of the layout, each against Python -> (bits, kinds, paths)"""
    bits, kinds, paths = tn._twin_values(twin, lay.data + lay.behind, lay.starts, len(lay.data))
    for c, s, b, k in zip(lay.cases, lay.starts, bits.tolist(), kinds.tolist()):
        assert lay.data[s:s + len(c.text)] == c.text and (s + len(c.text) == len(lay.data) or lay.data[s + len(c.text)] in b" ,]")
        assert (k, b) == tnm.expected(lay.data, s), (c.group, c.kind, c.phase)
    return bits, kinds, paths


def check_pairs_differ(lay, bits, kinds, count):
    """Every text with the far digit and its twin without: one byte apart, different bits -- a reader that misses that byte
    gives the twin's value"""
    where = {id(c): k for k, c in enumerate(lay.cases)}
    got = nph.pairs(lay.cases)
    assert len(got) == count
    for a, b in got:
        diff = [p for p in range(len(a.text)) if a.text[p] != b.text[p]]
        assert len(a.text) == len(b.text) and len(diff) == 1 and (a.text[diff[0]], b.text[diff[0]]) == (0x31, 0x30), (a, b)
        ka, kb = where[id(a)], where[id(b)]
        assert kinds[ka] == kinds[kb] == tnm.DOUBLE and bits[ka] != bits[kb], (a.group, a.kind, a.phase)


def test_corpus_on_cpu(twin):
    """The generator's promises, counted, and the host twin against Python on every text."""
    paths = np.zeros(3, dtype=np.uint64)
    # A: 7 kinds x 16 start residues x 4 window offsets, both signs; the feature at window offset o
    a = nph.group_a()
    assert len(nph.A_KINDS) == 7 and a.mod == 16
    per = Counter((c.kind, c.phase) for c in a.cases)
    assert per == {(k, (s, o)): cnt for k, cnt in A_TEXTS.items() for s in range(16) for o in (62, 63, 64, 65)}
    assert len(per) == (7 + 1) * PLACES and len(a.cases) == sum(A_TEXTS.values()) * PLACES == 1664
    for c, s in zip(a.cases, a.starts):
        check_a_case(c, s)
    assert sum(c.text[:1] == b"-" for c in a.cases) * 2 == len(a.cases)
    bits, kinds, p = twin_and_python(twin, a)
    paths += p
    check_pairs_differ(a, bits, kinds, 6 * PLACES)
    assert Counter(kinds.tolist()) == {tnm.DOUBLE: 1664 - 2 * PLACES, tnm.ERR_SYNTAX: 2 * PLACES}
    # B: every length with both endings, every residue of len with every class of lengths and either ending
    b = nph.group_b()
    assert len(b) == 292 and all(len(lay.cases) == 1 and lay.behind == b"7" * 64 for lay in b)
    for blank in (0, 1):
        mine = [lay for lay in b if lay.cases[0].phase[2] == blank]
        assert Counter(lay.cases[0].phase[1] for lay in mine) == {n: 2 for n in nph.B_LENGTHS} and len(nph.B_LENGTHS) == 73
        for lo, hi in ((1, 15), (17, 48), (65, 90)):
            assert {lay.cases[0].phase[0] for lay in mine if lo <= lay.cases[0].phase[1] <= hi} == set(range(16))
    for lay in b:
        (res, n, blank), t = lay.cases[0].phase, lay.cases[0].text
        assert len(t) == n and len(lay.data) % 16 == res and lay.data.endswith(t + b" " * blank) and lay.data[:3] == b"[1,"
        _, kinds, p = twin_and_python(twin, lay)
        paths += p
        assert kinds[0] == (tnm.INT64 if n <= 18 else tnm.DOUBLE)
        # a reader that takes the '7' behind len for data gives another value
        assert blank or tnm.expected(lay.data + b"7", lay.starts[0]) != tnm.expected(lay.data, lay.starts[0]), lay.cases[0]
    # C: every kind at every r = 0 .. 63, the feature 64 k + r bytes behind the start of the walked run, k >= 1
    first, second = nph.group_c()
    assert first.mod == second.mod == 64 and max(len(first.data), len(second.data)) < 1 << 20
    phase_cases = [c for c in first.cases + second.cases if c.group == "C"]
    per = Counter((c.kind, c.phase) for c in phase_cases)
    kinds_c = [k for k in nph.C_KINDS if k not in C_PAIRED] + [k + z for k in C_PAIRED for z in ("", "0")]
    assert len(nph.C_KINDS) == 11 and per == {(k, r): 1 for k in kinds_c for r in range(64)} and len(phase_cases) == 14 * 64
    for c in phase_cases:
        assert 1024 < len(c.text) < 1300 and (c.text[:1] == b"-") == bool(c.phase & 1), (c.kind, c.phase, len(c.text))
        if c.kind == "mult64":
            assert mult64_run(c) % 64 == 0 and mult64_run(c) >= 1024
        elif not c.kind.endswith("0"):   # (a twin: one byte apart from the case in front of it, check_pairs_differ)
            run, at = run_and_feature(c)
            assert at - run >= 64 and (at - run) % 64 == c.phase, (c.kind, c.phase, run, at)
    assert Counter(nph.MULT64_FORMS[c.phase % 4] for c in phase_cases if c.kind == "mult64") == {f: 16 for f in nph.MULT64_FORMS}
    # C-threshold: every kind (mult64 in its four forms) at r = 0 in 1 023 .. 1 026 characters
    per = Counter((c.kind, c.phase) for c in second.cases if c.group == "C-threshold")
    assert per == {(k, n): 4 if k == "mult64" else 1 for k in kinds_c for n in (1023, 1024, 1025, 1026)}
    for c in second.cases:
        if c.group == "C-threshold":
            assert len(c.text) == c.phase
            if c.kind == "mult64":
                assert mult64_run(c) % 64 == 0
            elif not c.kind.endswith("0"):
                run, at = run_and_feature(c)
                assert at - run >= 64 and (at - run) % 64 == 0, (c.kind, c.phase)
    # C-start: a long number at every residue of the buffer; and the first array holds more long numbers than num_long has waves
    starts = [(c, s) for c, s in zip(first.cases, first.starts) if c.group == "C-start"]
    assert [s % 64 for _, s in starts] == list(range(64)) and all(len(c.text) > 1024 for c, _ in starts)
    assert {c.group for c in first.cases} == {"C", "C-start"} and {c.group for c in second.cases} == {"C", "C-threshold"}
    assert len(first.cases) == 9 * 64 > nph.LONG_WAVES and all(len(c.text) > 1024 for c in first.cases)
    for lay, n_pairs in ((first, 0), (second, 3 * 64 + 3 * 4)):
        assert [s % 64 for s in lay.starts] == list(lay.residues)
        bits, kinds, p = twin_and_python(twin, lay)
        paths += p
        check_pairs_differ(lay, bits, kinds, n_pairs)
        assert int((kinds == tnm.ERR_SYNTAX).sum()) == sum(c.kind == "frac_x" for c in lay.cases) and not (kinds == tnm.ERR_RANGE).any()
    # C-end: the walked run ends at len, 64 * 17 + m bytes behind its start
    e = nph.group_c_end()
    assert Counter((lay.cases[0].kind, lay.cases[0].phase) for lay in e) == {(k, m): 1 for k in ("exp", "tie") for m in range(64)}
    for lay in e:
        c, s = lay.cases[0], lay.starts[0]
        run = s + (_exponent_digits(c.text) if c.kind == "exp" else c.text.index(b".") + 1)
        assert len(lay.data) - run == 64 * 17 + c.phase and lay.data.endswith(c.text) and nph.is_long(c.text, s, len(lay.data))
        _, _, p = twin_and_python(twin, lay)
        paths += p
        assert tnm.expected(lay.data + b"7", s) != tnm.expected(lay.data, s), c.kind
    assert len({lay.starts[0] % 64 for lay in e}) >= 32
    # D: the exact-path numbers are the capacity of the array's own n, - 1, + 0, + 1
    for delta, (data, slow, count) in nph.group_d().items():
        assert data.count(b",") == count - 1 and slow == nph.fallback_capacity(2 * count + 1) + delta and count - slow >= 5
        texts = data[1:-1].split(b",")
        kinds, _, p = tnm.convert_all(twin, texts)
        assert p.tolist() == [count - slow, 0, slow] and set(kinds.tolist()) == {tnm.INT64, tnm.DOUBLE}
    assert (paths > 0).all(), paths.tolist()   # fast, Eisel-Lemire, exact


# ---- on the device ----------------------------------------------------------------------------------------------------------

def check_layout(dev, twin, lay, where, pairs=False):
    """One call of stage 1, spans and numbers over the layout (tests/test_numbers._check_call: every record against the
    twin and Python, the counts, n_slow against the twin's exact-path count); then the start of every case from idx, its
    residue, and MSJ_SPAN_LONG on exactly the numbers of 1 025 characters and more.  -> (kinds, result, long flags)"""
    seen = {}
    _, tokens, kinds, res = tn._check_call(dev, twin, lay.data, where, behind=lay.behind, pairs=pairs, seen=seen)
    assert seen["address"] % 16 == 0
    k = len(lay.cases)
    starts = seen["idx"][seen["num_tok"]][-k:]
    assert starts.tolist() == list(lay.starts) and (starts % lay.mod).tolist() == list(lay.residues), where
    assert res.n_numbers == k + (1 if lay.behind else 0), where   # (the 1 of "[1," in front of a last token)
    long_flags = (seen["flags"][seen["num_tok"]][-k:] & LONG) != 0
    assert long_flags.tolist() == [nph.is_long(c.text, s, len(lay.data)) for c, s in zip(lay.cases, lay.starts)], where
    return kinds[-k:], res, long_flags


def _span_call(dev, request, mode):
    dev.lib.msj_debug_set_span_mode(dev.ctx, mode)
    request.addfinalizer(lambda: dev.lib.msj_debug_set_span_mode(dev.ctx, 0))


@pytest.mark.gpu
@pytest.mark.parametrize("call,mode", SPAN_CALLS)
def test_lane_window(dev, twin, request, call, mode):
    """Group A: the feature at window offsets 62 .. 65 for every start residue; the flags from the span call or from
    msj_stage2_prep_pairs_device, by the density of the index or with either span kernel forced."""
    _span_call(dev, request, mode)
    a = nph.group_a()
    kinds, res, long_flags = check_layout(dev, twin, a, ("A", call, mode), pairs=call == "pairs")
    assert not long_flags.any()
    bad = [k for k, c in enumerate(a.cases) if c.kind == "x"]
    assert (res.n_numbers, res.n_errors, res.first_error) == (len(a.cases), len(bad), 1 + 2 * bad[0])
    assert res.n_slow > 0


@pytest.mark.gpu
def test_end_of_the_buffer(dev, twin):
    """Group B: the number as the last token, the byte-by-byte chunk of the window as its first, a middle or its last one or
    none of them, '7' in the 64 bytes behind len."""
    for lay in nph.group_b():
        kinds, res, long_flags = check_layout(dev, twin, lay, ("B",) + lay.cases[0].phase)
        assert (res.n_numbers, res.n_errors, res.first_error) == (2, 0, UINT64_MAX) and not long_flags.any()


@pytest.mark.gpu
@pytest.mark.parametrize("call,mode", SPAN_CALLS)
def test_wave_steps(dev, twin, request, call, mode):
    """Group C: the feature at every lane of a 64-byte step, C-threshold, C-start.  The first array holds more long numbers
    than num_long has waves: its loop takes a second trip."""
    _span_call(dev, request, mode)
    for name, lay in zip(("first", "second"), nph.group_c()):
        kinds, res, long_flags = check_layout(dev, twin, lay, ("C", name, call, mode), pairs=call == "pairs")
        bad = [k for k, c in enumerate(lay.cases) if c.kind == "frac_x"]
        assert (res.n_numbers, res.n_errors, res.first_error) == (len(lay.cases), len(bad), 1 + 2 * bad[0])
        if name == "first":
            assert int(long_flags.sum()) == len(lay.cases) >= 513
        else:
            at = {(c.kind, c.phase): bool(f) for c, f in zip(lay.cases, long_flags) if c.group == "C-threshold" and c.kind != "mult64"}
            assert all(f == (n >= 1025) for (_, n), f in at.items()) and len(at) == 13 * 4
            assert res.n_slow > 0


@pytest.mark.gpu
def test_long_numbers_at_the_end_of_the_buffer(dev, twin):
    """C-end: a long number as the last token, len 0 .. 63 bytes behind the start of the reader's last step, '7' behind len."""
    for lay in nph.group_c_end():
        kinds, res, long_flags = check_layout(dev, twin, lay, ("C-end", lay.cases[0].kind, lay.cases[0].phase))
        assert (res.n_numbers, res.n_errors, res.first_error) == (2, 0, UINT64_MAX) and long_flags.all()
        assert kinds.tolist() == [tnm.DOUBLE]


@pytest.mark.gpu
def test_fallback_list_filled_exactly(dev, twin):
    """Group D: capacity - 1, capacity and capacity + 1 numbers that need the exact path, the capacity that of the call's own
    n: num_fallback resolves the first two lists, the overflow sweep the third; n_slow counts them either way."""
    dev.lib.msj_number_fallback_capacity.restype = ctypes.c_uint32
    dev.lib.msj_number_fallback_capacity.argtypes = [ctypes.c_uint64]
    for delta, (data, slow, count) in nph.group_d().items():
        seen = {}
        _, _, _, res = tn._check_call(dev, twin, data, ("D", delta), seen=seen)
        n = seen["idx"].size
        assert n == 2 * count + 1 and slow == dev.lib.msj_number_fallback_capacity(n) + delta
        assert (res.n_numbers, res.n_errors, res.n_slow) == (count, 0, slow)


@pytest.mark.gpu
def test_capacity_ends_at_a_listed_number(dev, twin):
    """The record list ends one record short of a long number's slot, and of an exact-path number's (and with that slot as
    its last): the list kernels store nothing at or behind `capacity`, the counts are those of the full call."""
    import torch

    data, k_long, k_slow = nph.clipped()
    seen = {}
    _, tokens, kinds, rf = tn._check_call(dev, twin, data, "clipped", seen=seen)
    assert seen["flags"][tokens[k_long]] & LONG and not seen["flags"][tokens[k_slow]] & LONG
    _, _, paths = tn._twin_values(twin, data, seen["idx"][tokens[k_slow:k_slow + 1]])
    assert paths.tolist() == [0, 0, 1] and rf.n_errors == 2 and rf.n_slow >= 4
    d_buf, d_idx, n, d_flags = tn._on_device(dev, data)
    full, _ = dev.number_values(d_buf, len(data), d_idx, n, d_flags)
    canary = 0x5A5A5A5A5A5A5A5A
    for cap in (k_long, k_long + 1, k_slow, k_slow + 1):
        d_num = torch.full((cap + 8, 2), canary, dtype=torch.int64, device=dev.device)
        _, rp = dev.number_values(d_buf, len(data), d_idx, n, d_flags, capacity=cap, d_numbers=d_num)
        assert (rp.n_numbers, rp.n_errors, rp.first_error, rp.n_slow) == (rf.n_numbers, rf.n_errors, rf.first_error, rf.n_slow), cap
        assert torch.equal(d_num[:cap], full[:cap]) and bool((d_num[cap:] == canary).all()), cap
