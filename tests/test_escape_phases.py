"""Every wave walk over a long escaped body -- wave_unescape (csrc/wave_unescape.h: msj_tape_device,
msj_tape_documents_device, msj_string_column_device) and wave_body_bad / wave_run_parity_before (csrc/validate_block.h:
msj_validate_device, msj_validate_documents_device) -- with an escape at EVERY phase of the 64-byte steps, in front of the
closing quote with a partial last step, and around the 4 096-byte piece borders of a body that the grid walks.

The corpus is tests/escape_phases.py.  The references are Python's: json.loads for valid text, tests/tape_reference.py for
the tape, the serial walker tests/test_validate_math.walk for the verdicts; the host twins give the whole-array comparisons
with fill and canaries.  test_corpus_on_cpu pins the corpus and the twins against Python before any GPU sees them.  Nothing
here is new machinery: the windows go through the helpers of tests/test_window_scale.py and tests/test_string_column.py,
the one-document calls through run_batch of tests/test_tape.py and tests/test_validate.py.
"""
import functools
import json

import numpy as np
import pytest

from tests import escape_phases as ep
from tests import helpers
from tests import tape_reference as ref
from tests import test_number_math as tnm
from tests import test_select_math as tsm
from tests import test_string_column as tsc
from tests import test_string_column_math as tcm
from tests import test_tape as tt
from tests import test_tape_documents_math as tdk
from tests import test_tape_math as ttm
from tests import test_validate as tv
from tests import test_validate_math as tvm
from tests import test_window_scale as tws

UINT64_MAX = tvm.UINT64_MAX
N_PHASE, N_END = 128, 84      # places per kind: 64 phases x 2 pads; 12 lengths of the last step x 7 distances from the quote


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
def env(dev):
    return tsc.Env(dev)


def verdict_of(case):
    """walk's verdict as a row of the one-document call: (code, token), (0, UINT64_MAX) for a valid line"""
    code, token = case.verdict
    return (code, UINT64_MAX if code == 0 else token)


@functools.lru_cache(maxsize=None)
def windows():
    """-> (valid, mixed): the two NDJSON windows as tws.Expected (the oracles' arrays and the verdict twin's rows), with the
    cases behind them as .cases"""
    out = []
    for cases in ep.corpus():
        lines = [c.line for c in cases]
        x = tws.Expected(b"\n".join(lines) + b"\n", lines)
        x.cases = cases
        out.append(x)
    return tuple(out)


def check_window_input(x):
    """The window's rows are walk's verdicts, document by document (the string's token counted from the window's first)"""
    w = x.w
    assert w.D == len(x.cases) and w.n == 5 * w.D and len(x.data) < 8 << 20
    first = w.first[:w.D].tolist()
    want = [(c.verdict[0], UINT64_MAX if c.verdict[0] == 0 else first[k] + c.verdict[1]) for k, c in enumerate(x.cases)]
    assert x.rows == want, [(k, g, v) for k, (g, v) in enumerate(zip(x.rows, want)) if g != v][:5]
    strings = np.nonzero(w.typ == ord('"'))[0][1::2]
    sizes = w.end[strings].astype(np.int64) - w.idx[strings] - 1
    assert strings.size == w.D and int(sizes.min()) > ep.LANE_BODY and bool(((w.flags[strings] & 2) != 0).all())


def column_rows(x):
    """What Python says of the column "/s": the UTF-8 of json.loads(line)["s"] for a valid line, None for an invalid one"""
    return [c.value["s"].encode("utf-8") if c.valid else None for c in x.cases]


def test_corpus_on_cpu():
    """The generator's promises, counted: every kind at all 64 phases with both pads (12 valid and 8 invalid kinds x 128
    places) and at 84 places in front of the closing quote, every body over 1 024 bytes, every invalid line followed by its
    sibling.  walk gives 0 for every valid line and the string error at the body's token for every invalid one.  The host
    twins agree with Python on the whole corpus: the verdict twin's rows are walk's, every document the tape twin builds
    decodes to json.loads of its line, the string-column twin's rows are the UTF-8 of the values."""
    valid, mixed = ep.corpus()
    assert len(ep.VALID) == 12 and len(ep.INVALID) == 8 and len(ep.INVALID_AT_END) == 1
    assert len(valid) == 12 * (N_PHASE + N_END) and len(mixed) == 2 * (8 * (N_PHASE + N_END) + 12)
    for cases, kinds in ((valid, ep.VALID), ([c for c in mixed if not c.sibling], ep.INVALID)):
        for kind, escape in kinds:
            mine = [c for c in cases if c.kind == kind]
            for carried in (False, True):
                phases = sorted(c.phase for c in mine if c.family == "phase" and (c.pad >= ep.CARRIED) == carried)
                assert phases == list(range(64)), (kind, carried, phases)
            assert all(c.tail >= 70 and c.pad in (c.phase, ep.CARRIED + c.phase) for c in mine if c.family == "phase")
            ends = sorted((len(c.line) - 8 - ep.CARRIED, c.tail) for c in mine if c.family == "end")
            assert ends == [(m, t) for m in range(1, 13) for t in range(7)], (kind, ends[:5])
    cut = [c for c in mixed if c.kind == "cut" and not c.sibling]
    assert sorted(len(c.line) - 8 - ep.CARRIED for c in cut) == list(range(1, 13)) and all(c.line.endswith(b'\\u00e"}') for c in cut)
    for c in valid + mixed:
        body = c.line[6:-2]
        assert c.line == ep.line_of(body) and len(body) > ep.LANE_BODY and body.count(b"\\") >= 1
        assert body[:c.pad] == b"x" * c.pad and body[c.pad] == 0x5C and body.endswith(b"y" * c.tail)
        if c.valid:
            assert c.verdict == (tvm.SUCCESS, None) and c.value == json.loads(c.line) and isinstance(c.value["s"], str), c.line[-40:]
        else:
            assert c.verdict == (tvm.STRING, ep.STRING_TOKEN) and c.value is None, (c.kind, c.pad, c.tail)
            if c.kind in ("q", "u00g9", "cut"):   # (json.loads passes lone surrogate halves through: walk decides those)
                assert not tvm.python_accepts(c.line), (c.kind, c.pad, c.tail)
    for k in range(0, len(mixed), 2):   # the sibling: the same place, € in the escape's place
        bad, good = mixed[k], mixed[k + 1]
        assert not bad.valid and not bad.sibling and good.valid and good.sibling and (good.pad, good.tail, good.kind) == (bad.pad, bad.tail, bad.kind)
        assert good.line == ep.line_of(ep.body_of(bad.pad, ep.SIBLING, bad.tail))
    assert len(ep.one_document_subset()) == 20 * (18 + N_END) + 12

    tm, stwin, ctwin = ttm.load_twin(), tsm.load_twin(), tcm.load_twin()
    for x, verdicts in zip(windows(), (False, True)):
        check_window_input(x)                                       # the verdict twin against walk
        built = tdk.twin_window(tdk.load_twin(), x.w, verdicts=x.rows if verdicts else None)
        tws.check_documents(x, built, range(x.w.D), [c.value for c in x.cases])   # the tape twin against json.loads
        records = tsm.twin_select(stwin, x.w, ["/s"], verdicts=x.rows if verdicts else None).column(0)[:x.w.D].copy()
        col = tcm.twin_column(ctwin, x.data, records, x.w.D)
        assert col.rows() == column_rows(x)                          # the string-column twin against json.loads
        assert col.res.n_escaped == col.res.n_strings == sum(c.valid for c in x.cases)
    # the one-document tape twin's string bytes against the serial reference, on the subset of the one-document calls
    oracle, nm = helpers.load_oracle(), tnm.load_twin()
    for c in ep.one_document_subset()[::7]:
        if c.valid:
            a = ttm.host_arrays(oracle, nm, c.line)
            ttm.check_twin_equals_reference(tm, c.line, a, *ref.build(c.line, a["idx"]))


# ---- the window calls ----------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_window_verdicts(dev):
    """msj_validate_documents_device over the valid window and over the mixed one, the oracles' arrays and the real chain:
    every row is walk's verdict (vd_strings: wave_body_bad with the escape at every phase)."""
    for x in windows():
        check_window_input(x)
        for chain in (False, True):
            res = tws.window_verdicts(dev, x, chain, where=chain)
            assert (res.n_invalid, res.n_escaped) == (sum(not c.valid for c in x.cases), x.w.D)


@pytest.mark.gpu
def test_window_tapes(dev):
    """msj_tape_documents_device over the valid window and, with the verdicts given, over the mixed one, both ways in: the
    result, records, tape and string buffer are the twin's, canaries included, and every built document decodes to
    json.loads of its line (td_long_out: wave_unescape writing).  The layout-only form runs wave_unescape measuring only."""
    valid, mixed = windows()
    for x, verdicts in ((valid, False), (mixed, True)):
        check_window_input(x)
        values = [c.value for c in x.cases]
        for chain in (False, True):
            got = tws.window_tape(dev, x, chain, verdicts=verdicts or chain, where=(verdicts, chain))
            assert got.res.n_built == sum(c.valid for c in x.cases)
            tws.check_documents(x, got, range(x.w.D), values)
        lay = tws.window_tape(dev, x, chain=True, verdicts=True, strings=False, where="layout only")
        assert lay.summary() == got.summary() and np.array_equal(lay.tape, got.tape)


@pytest.mark.gpu
def test_window_string_columns(env):
    """"/s" selected, then msj_string_column_device (sc_lengths: wave_unescape measuring; sc_copy: writing): offsets,
    validity and bytes are the twin's, whole arrays, layout-only and with bytes, both ways in; every valid row is the UTF-8
    of json.loads(line)["s"], every invalid one is no row."""
    for x, verdicts in zip(windows(), (False, True)):
        lines = [c.line for c in x.cases]
        for chain in (False, True):
            want, _ = tsc.check(env, lines, chain, verdicts=verdicts, where=(verdicts, chain))
        assert want.rows() == column_rows(x) and want.res.n_escaped == sum(c.valid for c in x.cases)


# ---- the one-document calls ----------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_one_document_verdicts(dev):
    """msj_validate_device (val_strings) on every kind at the phases 52 .. 63 and 0 .. 5 of the carried pad and on all of
    family "end": the code and the error token are walk's (run_batch holds each against the twin as well)."""
    cases = ep.one_document_subset()
    oracle, nm, twin = helpers.load_oracle(), tnm.load_twin(), tvm.load_twin()
    out = tv.run_batch(dev, twin, [(c.line, tv.host_arrays(oracle, nm, c.line), 100, True) for c in cases])
    want = [verdict_of(c) for c in cases]
    assert out == want, [(c.kind, c.pad, c.tail, g, v) for c, g, v in zip(cases, out, want) if g != v][:5]
    for c in cases[::97]:   # and the real chain
        r = tv.check_document(dev, oracle, twin, nm, c.line, where=(c.kind, c.pad))
        assert (r.code, r.error_token) == verdict_of(c)


@pytest.mark.gpu
def test_one_document_tapes(dev):
    """msj_tape_device (tape_long_len / tape_long_out) on the valid cases of the same subset: every word and every string
    byte are the twin's (run_batch) and the serial reference's, with the string buffer and in the layout-only form."""
    cases = [c for c in ep.one_document_subset() if c.valid]
    oracle, nm, tm = helpers.load_oracle(), tnm.load_twin(), ttm.load_twin()
    items = [(c.line, tt.arrays_of(oracle, nm, c.line), {}) for c in cases]
    out = tt.run_batch(dev, tm, items)
    for c, (_, a, _), (res, tape, sbuf) in zip(cases, items, out):
        w_tape, w_sbuf = ref.build(c.line, a["idx"])
        assert (res.code, res.n_strings) == (0, 2) and tape.tolist() == w_tape and sbuf.tobytes() == w_sbuf, (c.kind, c.pad, c.tail)
    for (res, tape, _), (res2, tape2, _) in zip(out, tt.run_batch(dev, tm, items, strings=False)):
        assert res2.code == 0 and res2.string_bytes == res.string_bytes and np.array_equal(tape, tape2)
    for c in cases[::97]:   # and the real chain
        assert tt.check_chain(dev, oracle, tm, nm, c.line).to_python() == c.value


# ---- the piece borders of a body that the grid walks ---------------------------------------------------------------------------

def check_huge_input(line):
    """The body is over kWaveBody and cut into pieces of 4 096 bytes: with 512 blocks of 4 waves a piece would be 576"""
    size = len(line) - 8
    assert size == ep.HUGE > ep.WAVE_BODY and ((size + 2047) // 2048 + 63) & ~63 < ep.PIECE


@pytest.mark.gpu
def test_piece_borders_valid(env):
    """One body of 1 MiB + 4 097 bytes with every valid kind starting -12 .. +6 bytes from a piece border of its own:
    msj_validate_device and msj_validate_documents_device give 0; the tape of it and the string column over it are
    Python's."""
    dev = env.dev
    line, places = ep.huge_valid()
    check_huge_input(line)
    assert sorted((k, d) for k, d, _, _ in places) == sorted((k, d) for k, _ in ep.VALID for d in range(-12, 7))
    assert len({b for _, _, b, _ in places}) == len(places) == 12 * 19
    assert all(line[6 + at:6 + at + len(ep.ESCAPES[k])] == ep.ESCAPES[k] and at == b * ep.PIECE + d for k, d, b, at in places)
    value = json.loads(line)
    oracle, nm = helpers.load_oracle(), tnm.load_twin()
    idx = tvm.stage1(oracle, line)
    assert tvm.walk(line, idx.tolist()) == (tvm.SUCCESS, None)
    r = tv.check_document(dev, oracle, tvm.load_twin(), nm, line, where="huge")
    assert tv.quad(r) == (0, UINT64_MAX, UINT64_MAX, 0) and r.n_escaped == 1
    assert tt.check_chain(dev, oracle, ttm.load_twin(), nm, line).to_python() == value
    lines = [b'{"s":"a\\nb"}', line, b'{"s":"tail"}']
    x = tws.Expected(b"\n".join(lines) + b"\n", lines)
    assert x.codes == [0, 0, 0]
    for chain in (False, True):
        tws.window_verdicts(dev, x, chain, where=chain)
        got = tws.window_tape(dev, x, chain, verdicts=chain, where=chain)
        assert tws.document_of(got, 1).to_python() == value
        want, _ = tsc.check(env, lines, chain, where=chain)
    assert want.rows() == [b"a\nb", value["s"].encode("utf-8"), b"tail"]


@pytest.mark.gpu
def test_piece_borders_invalid(dev):
    """34 bodies of 1 MiB + 4 097 bytes with one bad escape each: \\ud83d\\u0041 and a lone low surrogate starting 11 .. 0
    bytes in front of a piece border (the pair's second half, or the escape 6 bytes in front, belongs to the neighbouring
    piece: scan_begin, prev_starts), \\q and \\u00g9 at -5, -1, 0, +1, +5.  Half of the bodies go through msj_validate_device,
    the rest as one window through msj_validate_documents_device (ep.huge_invalid says which: each call gets every delta
    -11 .. 0 from one of the two surrogate kinds, -6 and 0 among them): the string error at the body's token."""
    bodies = ep.huge_invalid()
    assert len(bodies) == 34 <= 40 and {b for _, _, b, _, _ in bodies} >= {1, 256}
    for one in (True, False):   # each call: every delta of the 12-long ranges, and \\q / \\u00g9 on both sides of a border
        mine = [(k, d) for k, d, _, o, _ in bodies if o == one]
        assert sorted(d for k, d in mine if k in ("high_bmp", "lone_low")) == list(range(-11, 1)) and len(mine) == 17
        assert {-6, 0} <= {d for k, d in mine if k == ("lone_low" if one else "high_bmp")}
        assert {d > 0 for k, d in mine if k in ("q", "u00g9")} == {True, False}
    assert sorted((k, d) for k, d, _, _, _ in bodies) == sorted((k, d) for k, ds in ep.INVALID_DELTAS.items() for d in ds)
    oracle, nm, twin = helpers.load_oracle(), tnm.load_twin(), tvm.load_twin()
    for kind, delta, border, _, line in bodies:
        check_huge_input(line)
        at = 6 + border * ep.PIECE + delta
        assert line[at:at + len(ep.ESCAPES[kind])] == ep.ESCAPES[kind] and line.count(b"\\") == ep.ESCAPES[kind].count(b"\\")
        assert tvm.walk(line, tvm.stage1(oracle, line).tolist()) == (tvm.STRING, ep.STRING_TOKEN), (kind, delta)
    for kind, delta, border, line in [(k, d, b, text) for k, d, b, one, text in bodies if one]:
        r = tv.check_document(dev, oracle, twin, nm, line, where=(kind, delta, border))
        assert (r.code, r.error_token) == (tvm.STRING, ep.STRING_TOKEN), (kind, delta, border, r.code, r.error_token)
    lines = [b'{"s":"ok"}'] + [line for _, _, _, one, line in bodies if not one]
    x = tws.Expected(b"\n".join(lines) + b"\n", lines)
    first = x.w.first[:x.w.D].tolist()
    assert x.rows == [(0, UINT64_MAX)] + [(tvm.STRING, f + ep.STRING_TOKEN) for f in first[1:]]
    for chain in (False, True):
        tws.window_verdicts(dev, x, chain, where=chain)
