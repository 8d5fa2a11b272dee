"""The per-window calls -- msj_validate_documents_device, msj_tape_documents_device, msj_select_documents_device -- at the
sizes where their launches wrap: more blocks than the scan takes in one chunk, more documents than the grid over the
documents has lanes, more number records and more long bodies than the list kernels have lanes and waves, and a container
that climbs every level of the minimum tree inside a window of several documents.  And the column calls --
msj_string_column_device, msj_array_column_device -- past their grids: more blocks of rows than sc_scan takes in one chunk,
more rows than sc_lengths / sc_copy and ac_rows reach in one trip, a block whose rows are all long escaped bodies.

Nothing here is new machinery: the windows' arrays (tdm.WindowArrays), the host twins (tdm.twin_documents, tdk.twin_window,
tsm.twin_select), the two ways in (Uploaded / FromChain), the device calls and the whole-array comparisons are those of
tests/test_validate_documents.py, tests/test_tape_documents.py, tests/test_select_documents.py, tests/test_string_column.py and
tests/test_array_column.py, and the one-document calls go through tests/test_tape.py, tests/test_validate.py and
tests/test_numbers.py.  Every comparison is exact.  Every test
asserts that its input is past the threshold it is named for.  The constants below are mirrors of the kernels' values,
written by hand: a constant changed here makes the test fail and not pass on an input that no longer reaches it; a constant
changed in a kernel has to be changed here too.  The expected values of a window are computed once and shared.
"""
import functools
import json
import random

import numpy as np
import pytest

from mojo_simdjson_amd.document import Document
from tests import escape_phases as ep
from tests import helpers
from tests import tape_reference
from tests import test_array_column as tacd
from tests import test_array_column_math as tac
from tests import test_number_math as tnm
from tests import test_numbers as tnum
from tests import test_select_documents as tsd
from tests import test_select_math as tsm
from tests import test_string_column as tsc
from tests import test_string_column_math as tcm
from tests import test_tape as tt
from tests import test_tape_documents as ttd
from tests import test_tape_documents_math as tdk
from tests import test_tape_math as ttm
from tests import test_validate as tv
from tests import test_validate_documents as tvd
from tests import test_validate_documents_math as tdm
from tests import test_validate_math as tvm

BLOCK = 1024                 # tape_block.h: kBlock = kThreads * kPer, the tokens of a workgroup
SCAN_BLOCKS = 1024           # tape_block.h, scan_blocks: `for (b0 = 0; b0 < w.nb; b0 += 1024)`, blocks per chunk of the running carry
DOC_GRID = 1024 * 256        # docs_block.h: row_grid_blocks / validate_docs_kernel.hip: kGridBlocks = 1024 blocks of kThreads = 256 lanes along k
RECORD_LANES = 512 * 256     # validate_docs_kernel.hip: vd_records is launched with dim3(kListBlocks) = 512 blocks of kThreads lanes
LIST_WAVES = 512 * 4         # tape_block.h / validate_block.h: kListBlocks = 512 blocks of kWaves = 4 waves, `j += waves`
NUM_LONG_WAVES = 128 * 4     # numbers_kernel.hip: num_long is launched with dim3(kListBlocks / 4) = 128 blocks of 4 waves
ROW_BLOCK = 256              # string_column_kernel.hip: kRows, the rows of a workgroup of sc_lengths / sc_copy
ROW_GRID = 4096 * ROW_BLOCK  # string_column_kernel.hip: kGridBlocks = 4096 blocks of kRows rows, `v += gridDim.x`
LANE_BODY = 1024             # tape_block.h / validate_block.h: kLaneBody; numbers_kernel.hip: MSJ_SPAN_LONG is over 1024 characters

UINT64_MAX = tvm.UINT64_MAX
MSJ_CAPACITY = 1
SCALE_PATHS = ["/id", "/u/n", "", "/k", "/u", "/no"]
TREE_PATHS = ["/a", "/z", "/p/a", "/p/z/q", "/p/z"]


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
    return tsd.Env(dev)


class Expected:
    """A window with what the oracles and the verdict twin give for it, computed once: the arrays, the verdict rows with
    every number record and with d_numbers_result NULL, the codes"""

    def __init__(self, data, texts):
        self.data, self.texts = data, texts
        self.w = tdm.WindowArrays(helpers.load_oracle(), tnm.load_twin(), data, is_final=False)
        self.rows, self.res = tdm.twin_documents(tdm.load_twin(), self.w)
        self.codes = [c for c, _ in self.rows]
        self._unchecked = None

    def unchecked(self):
        if self._unchecked is None:
            self._unchecked = tdm.twin_documents(tdm.load_twin(), self.w, numbers="none")
        return self._unchecked


def window_tape(dev, x, chain, verdicts, strings=True, where=None):
    """msj_tape_documents_device over the window `x` against the twin, whole arrays and canaries -> the device's tdk.Built"""
    rows = x.rows if verdicts else None
    want = tdk.twin_window(tdk.load_twin(), x.w, verdicts=rows, strings=strings, canary=ttd.CANARY)
    a = ttd.FromChain(dev, x.data, False, verdicts) if chain else ttd.Uploaded(dev, x.w, rows)
    assert a.n == x.w.n, where
    got = ttd.device_window(a, want.caps, strings=strings)
    ttd.same(got, want, where)
    return got


def window_select(env, x, pointers, chain, verdicts, capacity, want=None, where=None):
    """msj_select_documents_device over the window `x` against the twin, the whole d_fields array -> the device's tsm.Selected"""
    rows = x.rows if verdicts else None
    if want is None:
        want = tsm.twin_select(env.stwin, x.w, pointers, verdicts=rows, capacity=capacity)
    a = tsd.FromChain(env.dev, x.data, False, verdicts) if chain else tsd.Uploaded(env.dev, x.w, rows)
    assert a.n == x.w.n, where
    got = tsd.device_select(a, env.paths(pointers), want.capacity)
    tsd.same(got, want, where)
    return got


def verdict_arrays(dev, x, chain):
    """The window's arrays for the verdict call: the real chain on the device, else the oracles' arrays uploaded"""
    a = tvd.Chain(dev, x.data) if chain else tsd.Uploaded(dev, x.w, None)
    assert a.n == x.w.n, chain
    return a


def window_verdicts(dev, x, chain, numbers=True, capacity=None, where=None, a=None):
    """msj_validate_documents_device over the window `x` (a: its arrays if the caller has them, verdict_arrays) against the
    twin: every row, the rows behind them untouched (tvd.unpack), and the result -> the result"""
    a = verdict_arrays(dev, x, chain) if a is None else a
    want, wres = (x.rows, x.res) if numbers else x.unchecked()
    got, res = tvd.device_verdicts(a, numbers=numbers, capacity=x.w.D if capacity is None else capacity)
    assert tvd.summary(res) == tvd.summary(wres), (where, tvd.summary(res), tvd.summary(wres))
    assert got == want, (where, [(k, g, v) for k, (g, v) in enumerate(zip(got, want)) if g != v][:5])
    return res


def document_of(built, k):
    """Document k of a tdk.Built from its record alone: its slice of the tape and of the string buffer"""
    r = built.recs[k]
    t0, s0 = int(r["tape_first"]), int(r["string_first"])
    return Document(built.tape[t0:t0 + int(r["tape_words"])], built.sbuf[s0:s0 + int(r["string_bytes"])])


# ---- 1. one NDJSON window past the document grid and the scan chunk ----------------------------------------------------------

SCALE_LINES = DOC_GRID + 1500


def scale_window():
    """-> (data, lines): SCALE_LINES lines of NDJSON.  Most are {"id":N}; every fifth has an escaped string, a float and a
    nested object; every 1 000th, at offset 7, is structurally invalid and, at offset 13, holds a bad number; line 3 has a
    duplicate key."""
    lines = []
    for n in range(SCALE_LINES):
        if n == 3:
            lines.append(b'{"id":"dup","id":2}')
        elif n % 1000 == 7:
            lines.append(b'{"id":%d,"a":[1,2,tru]}' % n)
        elif n % 1000 == 13:
            lines.append(b'{"id":01}')
        elif n % 5 == 0:
            lines.append(b'{"id":%d,"u":{"n":"x\\n%d"},"k":-1.5e3}' % (n, n))
        else:
            lines.append(b'{"id":%d}' % n)
    return b"\n".join(lines) + b"\n", lines


@functools.lru_cache(maxsize=None)
def scale():
    return Expected(*scale_window())


def straddler(w):
    """The document that holds the last token of the scan's first chunk"""
    return int(np.searchsorted(w.first[:w.D], SCAN_BLOCKS * BLOCK - 1, side="right")) - 1


def check_scale_input(x):
    """The window is past every threshold the tests over it are named for, and its mix is the one its generator describes"""
    w = x.w
    assert w.D == len(x.texts) == SCALE_LINES > DOC_GRID and w.T == w.n > SCAN_BLOCKS * BLOCK
    assert w.records.size > RECORD_LANES
    bad = np.nonzero(w.records["kind"] >= tnm.ERR_SYNTAX)[0]
    assert bad.size == w.n_errors == len(range(13, SCALE_LINES, 1000)) and int(bad[-1]) > RECORD_LANES
    f, e = w.bounds(straddler(w))
    assert f < SCAN_BLOCKS * BLOCK < e, (f, e)
    n_tru, n_num = len(range(7, SCALE_LINES, 1000)), len(range(13, SCALE_LINES, 1000))
    assert [x.codes.count(c) for c in (0, tvm.T_ATOM, tvm.NUMBER)] == [w.D - n_tru - n_num, n_tru, n_num]
    assert all(x.codes[k] == tvm.T_ATOM for k in range(7, w.D, 1000)) and all(x.codes[k] == tvm.NUMBER for k in range(13, w.D, 1000))
    assert sum(1 for t in x.texts if b'"u"' in t) == len(range(0, SCALE_LINES, 5))
    assert (x.res.n_invalid, x.res.first_invalid, x.res.flags) == (n_tru + n_num, 7, 0)


@functools.lru_cache(maxsize=None)
def scale_selected():
    """The select twin over the scale window with the verdicts given and a capacity that is not D, held against the
    definition (tests/select_reference.py) on every document -> (Selected, {(p, k): (code, value)})"""
    x = scale()
    want = tsm.twin_select(tsm.load_twin(), x.w, SCALE_PATHS, verdicts=x.rows, capacity=x.w.D + 37)
    return want, tsm.check_against_reference(x.w, want, SCALE_PATHS, x.texts, codes=x.codes)


def test_scale_window_on_cpu():
    """The generator's conditions, and the three twins against Python on every line of the scale window: a verdict is 0
    exactly when json.loads takes the line, every field is the reference's, and every valid line's slice of the tape twin's
    arrays is a self-contained Document that decodes to json.loads of the line (an invalid line's record has the verdict's
    code and zero sizes).  This pins the expected values before any GPU sees them."""
    x = scale()
    check_scale_input(x)
    values = []
    for k, line in enumerate(x.texts):
        try:
            values.append(json.loads(line))
            taken = True
        except ValueError:
            values.append(None)
            taken = False
        assert (x.codes[k] == 0) == taken, (k, line)
    want, out = scale_selected()
    assert out[(0, 3)] == (0, "dup") and out[(1, 5)] == (0, "x\n5") and out[(3, 5)] == (0, -1500.0) and out[(5, 5)] == (20, None)
    assert want.res.n_found == sum(1 for c, _ in out.values() if c == 0)
    built = tdk.twin_window(tdk.load_twin(), x.w, verdicts=x.rows)
    assert built.res.n_built == x.w.D - int(x.res.n_invalid)
    check_documents(x, built, range(x.w.D), values)


def picked_documents(w):
    """The first and the last document, those around index DOC_GRID, the one across the scan's chunk border with its
    neighbours, the first lines of each special kind and a seeded sample of 2 000 more"""
    k = straddler(w)
    return sorted({0, w.D - 1, DOC_GRID - 1, DOC_GRID, DOC_GRID + 1, k - 1, k, k + 1, 3, 7, 13} | set(random.Random(20280).sample(range(w.D), 2000)))


def check_documents(x, built, picks, values=None):
    """Independently of the twin: each of the documents `picks` is a self-contained Document -- its record's slice of the
    tape and of the string buffer -- equal to json.loads of its line (values: those, if the caller has them); an invalid
    one has the verdict's code and zero sizes"""
    for k in picks:
        r = built.recs[k]
        assert int(r["code"]) == x.codes[k], (k, r)
        if x.codes[k]:
            assert (int(r["tape_words"]), int(r["string_bytes"])) == (0, 0), (k, r)
        else:
            want = json.loads(x.texts[k].decode("utf-8")) if values is None else values[k]
            assert document_of(built, k).to_python() == want, (k, x.texts[k])


@pytest.mark.gpu
def test_validate_documents_scale(dev):
    """More documents than vd_init / vd_finish have lanes, more number records than vd_records has lanes with bad ones among
    the later, binary searches in hundreds of thousands of starts: every row, n_invalid, first_invalid, n_escaped and the
    flags are the twin's, both ways in; without d_numbers_result the flag and no number error; one row short, MSJ_CAPACITY
    and no row written."""
    x = scale()
    check_scale_input(x)
    D = x.w.D
    for chain in (False, True):
        a = verdict_arrays(dev, x, chain)   # (one upload / one run of the chain for the three calls)
        res = window_verdicts(dev, x, chain, where=chain, a=a)
        assert (res.code, res.n_documents, res.n_escaped) == (0, D, len(range(0, D, 5)))
        res = window_verdicts(dev, x, chain, numbers=False, where=(chain, "unchecked"), a=a)
        assert (res.flags, res.n_invalid) == (tvm.NUMBERS_UNCHECKED, len(range(7, D, 1000)))
        got, res = tvd.device_verdicts(a, capacity=D - 1)   # (unpack: every row of d_verdicts still holds the fill)
        assert got == [] and (res.code, res.n_documents, res.n_invalid) == (MSJ_CAPACITY, D, 0)


@pytest.mark.gpu
def test_tape_documents_scale(dev):
    """More blocks than scan_blocks takes in one chunk, under td_scan's document layout, and a document across the chunk
    border: the result, every record, every tape word and every string byte are the twin's, canaries included -- the
    oracles' arrays with verdicts, the chain without, the layout-only form -- and the picked documents decode to their
    lines."""
    x = scale()
    check_scale_input(x)
    got = window_tape(dev, x, chain=False, verdicts=True, where="uploaded")
    assert got.res.n_built == x.w.D - int(x.res.n_invalid) and got.res.n_documents == x.w.D
    check_documents(x, got, picked_documents(x.w))
    free = window_tape(dev, x, chain=True, verdicts=False, where="chain, no verdicts")
    assert free.res.n_built == x.w.D
    lay = window_tape(dev, x, chain=True, verdicts=True, strings=False, where="layout only")
    assert lay.summary() == got.summary() and np.array_equal(lay.tape, got.tape)


@pytest.mark.gpu
def test_select_documents_scale(env):
    """More documents than the grid along k has lanes, six paths (blockIdx.y), and a capacity that is not D (the stride of
    the state words and of d_fields differ from D): the whole d_fields array is the twin's, fill and canary included, and
    that twin is the reference's on every document (scale_selected); n_found is the host count; line 3 gives "dup"."""
    x = scale()
    check_scale_input(x)
    D = x.w.D
    want, out = scale_selected()
    assert want.capacity == D + 37 and len(SCALE_PATHS) == 6
    got = window_select(env, x, SCALE_PATHS, chain=False, verdicts=True, capacity=D + 37, want=want, where="uploaded, D + 37")
    found = sum(int((got.column(p)[:D]["code"] == 0).sum()) for p in range(len(SCALE_PATHS)))
    assert got.res.n_found == found == sum(1 for c, _ in out.values() if c == 0)
    data = np.frombuffer(x.data, dtype=np.uint8)
    assert tsm.field_value(got.column(0)[3], data, x.w.idx, x.w.end) == "dup" == out[(0, 3)][1]
    got = window_select(env, x, SCALE_PATHS, chain=True, verdicts=True, capacity=D, where="chain, D")
    assert got.res.n_found == found and all(np.array_equal(got.column(p), want.column(p)[:D]) for p in range(len(SCALE_PATHS)))
    free = window_select(env, x, SCALE_PATHS, chain=True, verdicts=False, capacity=D + 37, where="chain, no verdicts")
    assert free.res.n_found > found   # (the invalid documents are looked up too)


# ---- 2. one document through every level of the minimum tree, inside a window ------------------------------------------------

SECOND_LEVEL, THIRD_LEVEL = 70_000, 4_200_000   # elements: more than 64 and more than 4 096 blocks of tokens


def tree_window():
    """-> (data, documents): 50 small documents, an array of SECOND_LEVEL elements in an object, 20 small ones, an array of
    THIRD_LEVEL elements two objects down with an object behind it, 20 small ones"""
    small = lambda k: [b'{"a":%d,"z":{"q":"s%d"}}' % (k, k), b'{"p":{"z":{"q":%d},"a":[%d,"x\\n"]}}' % (k, k), b"[%d,-2.5e3]" % k, b'"z"'][k % 4]
    zeros = lambda count: np.tile(np.frombuffer(b"0,", dtype=np.uint8), count).tobytes()[:-1]
    docs = [small(k) for k in range(50)] + [b'{"a":[' + zeros(SECOND_LEVEL) + b'],"z":1}'] + [small(k) for k in range(50, 70)]
    docs += [b'{"p":{"a":[' + zeros(THIRD_LEVEL) + b'],"z":{"q":2}}}'] + [small(k) for k in range(70, 90)]
    return b"\n".join(docs) + b"\n", docs


@functools.lru_cache(maxsize=None)
def tree():
    return Expected(*tree_window())


def count_field(word):
    return (int(word) >> 32) & 0xFFFFFF


@pytest.mark.gpu
def test_minimum_tree_in_a_window(env):
    """The commas of an array over more than 64 blocks and of one over more than 4 096 blocks climb the second and the
    third level of span_body / td_min64 to their bracket, with other documents in front, between and behind: the tape
    is the twin's, and the count fields by hand.  Every verdict is 0 (0xFFFFFF > 4 200 000: the element limit is not in
    play, so vd_count's verdict is not what is tested here).  Keys that lie millions of tokens behind their object's opening
    brace are found through d_match (is_member_of)."""
    x, dev = tree(), env.dev
    w = x.w
    assert w.D == len(x.texts) == 92 and w.T == w.n
    (f1, e1), (f2, e2) = w.bounds(50), w.bounds(71)
    assert (e1 - f1) // BLOCK > 64 and (e2 - f2) // BLOCK > 64 * 64 and f2 // BLOCK > 64
    assert tvm.MAX_ELEMENTS > THIRD_LEVEL
    assert x.codes == [0] * w.D and tvd.summary(x.res)[:5] == (0, 0, w.D, 0, UINT64_MAX)
    window_verdicts(dev, x, chain=True, where="tree")

    got = window_tape(dev, x, chain=False, verdicts=True, where="tree, uploaded")
    window_tape(dev, x, chain=True, verdicts=False, where="tree, chain")
    # document 50: r { "a" [ 0 0 ... ] "z" 1 1 } r -- the array's bracket is word 3
    t = got.tape[int(got.recs[50]["tape_first"]):][:int(got.recs[50]["tape_words"])]
    assert [int(t[p]) >> 56 for p in (1, 3)] == [ord("{"), ord("[")] and [count_field(t[p]) for p in (1, 3)] == [2, SECOND_LEVEL]
    assert t.size == 2 + 2 + 1 + 2 + 2 * SECOND_LEVEL + 3
    # document 71: r { "p" { "a" [ 0 0 ... ] "z" { "q" 2 2 } } } r -- the array's bracket is word 5, the last object's
    # lies behind the array's 2 words per element and its closing bracket
    t = got.tape[int(got.recs[71]["tape_first"]):][:int(got.recs[71]["tape_words"])]
    z = 5 + 2 * THIRD_LEVEL + 3
    assert [int(t[p]) >> 56 for p in (1, 3, 5, z)] == [ord(c) for c in "{{[{"]
    assert [count_field(t[p]) for p in (1, 3, 5, z)] == [1, 2, THIRD_LEVEL, 1]
    for k in list(range(50)) + list(range(51, 71)) + list(range(72, 92)):   # (the Python walk: the small documents)
        assert document_of(got, k).to_python() == json.loads(x.texts[k].decode("utf-8")), k

    want = tsm.twin_select(env.stwin, w, TREE_PATHS, verdicts=x.rows)
    sel = window_select(env, x, TREE_PATHS, chain=False, verdicts=True, capacity=w.D, want=want, where="tree, uploaded")
    window_select(env, x, TREE_PATHS, chain=True, verdicts=False, capacity=w.D + 5, where="tree, chain")
    data = np.frombuffer(x.data, dtype=np.uint8)
    field = lambda p, k: (int(sel.column(p)[k]["code"]), tsm.field_value(sel.column(p)[k], data, w.idx, w.end))
    assert field(1, 50) == (0, 1) and field(3, 71) == (0, 2) and field(4, 71) == (0, {"q": 2}) and field(0, 71) == (20, None)
    for p, k, elements in ((0, 50, SECOND_LEVEL), (2, 71, THIRD_LEVEL)):   # the arrays: from the bracket to its partner
        r = sel.column(p)[k]
        first = int(r["token"])
        assert (int(r["code"]), chr(int(r["type"])), int(r["bits"]) - first) == (0, "[", 2 * elements)
    small = [k for k in range(w.D) if k not in (50, 71)]
    decoded = {k: tsm.ref.decode(x.texts[k]) for k in small}
    for p, pointer in enumerate(TREE_PATHS):
        for k in small:
            code, value = tsm.ref.lookup(decoded[k], pointer)
            assert field(p, k)[0] == code and tsm.same_value(field(p, k)[1], value), (pointer, k)


# ---- 3. lists longer than the grid that drains them --------------------------------------------------------------------------

def long_body(j, bad=False):
    """A body of 1 025 ... 1 100 bytes that names its number; every other one escaped (\\u20ac, \\n and a surrogate pair),
    ending in \\t -- or in \\q, which no string may hold"""
    size = LANE_BODY + 1 + j % 76
    if j % 2 == 0:
        return (b"plain %d " % j + b"abcdefghij" * 110)[:size]
    unit = b"\\u20ac\\n\\ud83d\\ude00e%d " % j
    body = unit * ((size - 2) // len(unit))
    return body + b"y" * (size - 2 - len(body)) + (b"\\q" if bad else b"\\t")


@functools.lru_cache(maxsize=None)
def body_window(count, bad=False):
    """`count` long bodies, each its own document ["..."], one window"""
    docs = [b'["' + long_body(j, bad) + b'"]' for j in range(count)]
    return Expected(b"\n".join(docs) + b"\n", docs)


def check_bodies(x, count, escaped_past_the_list):
    w = x.w
    strings = np.nonzero(w.typ == ord('"'))[0]
    sizes = w.end[strings].astype(np.int64) - w.idx[strings] - 1
    assert w.D == count and strings.size == count and int(sizes.min()) > LANE_BODY and int(sizes.max()) <= LANE_BODY + 76
    assert count > LIST_WAVES   # td_long_len / td_long_out / tape_long_len / tape_long_out: every long body is on their list
    if escaped_past_the_list:   # val_strings / vd_strings: the escaped ones are on theirs
        assert int(((w.flags[strings] & 2) != 0).sum()) > LIST_WAVES


@pytest.mark.gpu
def test_long_bodies_past_the_list_grid_in_a_window(dev):
    """More long bodies in one window than td_long_len / td_long_out have waves: every body's bytes are in the string
    buffer, so one that a loop skipped shows; every verdict is 0.  With twice as many, the escaped ones alone are more than
    vd_strings has waves."""
    x = body_window(LIST_WAVES + 100)
    check_bodies(x, LIST_WAVES + 100, escaped_past_the_list=False)
    assert x.codes == [0] * x.w.D
    for chain in (False, True):
        got = window_tape(dev, x, chain, verdicts=chain, where=chain)
        assert got.res.n_built == x.w.D and got.res.n_strings == x.w.D
        window_verdicts(dev, x, chain, where=chain)
    for k in (0, 1, LIST_WAVES - 1, LIST_WAVES, LIST_WAVES + 99):
        assert document_of(got, k).to_python() == json.loads(x.texts[k].decode("utf-8")), k
    twice = body_window(2 * (LIST_WAVES + 100))
    check_bodies(twice, 2 * (LIST_WAVES + 100), escaped_past_the_list=True)
    assert twice.codes == [0] * twice.w.D
    res = window_verdicts(dev, twice, chain=True, where="twice")
    assert res.n_escaped == LIST_WAVES + 100
    window_tape(dev, twice, chain=True, verdicts=True, where="twice")


@pytest.mark.gpu
def test_long_bodies_past_the_list_grid_in_one_document(dev, oracle):
    """The same bodies as ONE document [...] through msj_tape_device and msj_validate_device (tape_long_len, tape_long_out,
    val_strings), the oracles' arrays and the real chain, against their twins."""
    tm, nm, vt = ttm.load_twin(), tnm.load_twin(), tvm.load_twin()
    for count in (LIST_WAVES + 100, 2 * (LIST_WAVES + 100)):
        bodies = [long_body(j) for j in range(count)]
        data = b'["' + b'","'.join(bodies) + b'"]'
        a = tt.arrays_of(oracle, nm, data)
        assert int((a["typ"] == ord('"')).sum()) == count > LIST_WAVES and min(len(b) for b in bodies) > LANE_BODY
        (res, tape, sbuf), = tt.run_batch(dev, tm, [(data, a, {})])
        assert (res.code, res.n_strings) == (0, count)
        doc = tt.check_chain(dev, oracle, tm, nm, data)   # (every long body is on tape_long_len's / tape_long_out's list)
        assert doc.to_python() == json.loads(data.decode("utf-8"))
        if count > 2 * LIST_WAVES:   # the escaped ones alone are more than val_strings has waves
            assert int(((a["flags"] & 2) != 0).sum()) == count // 2 > LIST_WAVES
        arrays = tv.host_arrays(oracle, nm, data)
        assert tv.run_batch(dev, vt, [(data, arrays, 100, True)]) == [(0, UINT64_MAX)]
        got = tv.check_document(dev, oracle, vt, nm, data, where=count)
        assert tv.quad(got) == (0, UINT64_MAX, UINT64_MAX, 0) and got.n_escaped == count // 2


@pytest.mark.gpu
def test_bad_long_bodies_past_the_list_grid(dev):
    """Every escaped body ends in \\q, and there are more of them than vd_strings has waves: every such document's verdict is
    the string error at its token and every plain one's is 0.  Which slot of the list a body gets is decided by the order of
    the atomicAdds, so a single planted error could sit in the loop's first pass; with all of them bad, one drained in a
    later pass cannot hide."""
    for count in (LIST_WAVES + 100, 2 * (LIST_WAVES + 100)):
        x = body_window(count, bad=True)
        check_bodies(x, count, escaped_past_the_list=count > 2 * LIST_WAVES)
        first = x.w.first[:x.w.D].tolist()
        assert x.rows == [(tvm.STRING, first[k] + 1) if k % 2 else (0, UINT64_MAX) for k in range(count)]
        for chain in (False, True):
            res = window_verdicts(dev, x, chain, where=(count, chain))
            assert (res.n_invalid, res.first_invalid, res.n_escaped) == (count // 2, 1, count // 2)


def long_number(j):
    """A number of 1 025 ... 1 060 characters: an integer (a range error), 3.digits, -0.digits e-400, digits e-1050;
    every seventh ends in a letter"""
    size = LANE_BODY + 1 + j % 36
    digits = lambda count: (b"%d" % (j + 1) + b"1234567890" * 107)[:count]
    text = [digits(size), b"3." + digits(size - 2), b"-0." + digits(size - 8) + b"e-400", digits(size - 6) + b"e-1050"][j % 4]
    return text[:-1] + b"x" if j % 7 == 0 else text


@pytest.mark.gpu
def test_long_numbers_past_the_list_grid(dev):
    """More numbers of more than 1 024 characters in one call than num_long has waves: every record against the twin and
    against Python, n_errors and first_error against the records (tests/test_numbers.py: _check_call)."""
    count = NUM_LONG_WAVES + 40
    texts = [long_number(j) for j in range(count)]
    assert count > NUM_LONG_WAVES and all(LANE_BODY < len(t) <= LANE_BODY + 36 for t in texts)
    bits, tokens, kinds, res = tnum._check_call(dev, tnm.load_twin(), b"[" + b",".join(texts) + b"]", "long numbers")
    assert res.n_numbers == count and tokens.tolist() == list(range(1, 2 * count, 2))
    want = [tnm.ERR_SYNTAX if j % 7 == 0 else (tnm.ERR_RANGE, tnm.DOUBLE, tnm.DOUBLE, tnm.DOUBLE)[j % 4] for j in range(count)]
    assert kinds.tolist() == want and res.first_error == 1
    assert res.n_errors == sum(1 for k in want if k in tnum.ERRORS)


# ---- 4. the column calls past their grids ------------------------------------------------------------------------------------

def device_select_fields(env, x, pointers, capacity):
    """The real chain and the real select call over the window `x`, verdicts given, nothing waited for -> (arrays, d_sel, d_fields)"""
    a = tsd.FromChain(env.dev, x.data, False, True)
    assert a.n == x.w.n
    d_sel, d_fields = env.dev.select_documents(env.paths(pointers), a.d_buf, a.length, a.d_idx, a.n, a.d_type, a.d_depth, a.d_match, a.d_end,
                                               a.d_flags, a.d_first, a.d_docs, d_numbers=a.d_numbers, numbers_capacity=a.ncap,
                                               d_numbers_result=a.d_num, d_verdicts=a.d_verdicts, capacity=capacity, sync=False)
    return a, d_sel, d_fields


@pytest.mark.gpu
def test_string_column_second_scan_chunk(env):
    """msj_string_column_device over the scale window: 1 030 blocks of rows, more than the 1 024 block sums scan_in_place
    takes in sc_scan's first chunk.  "/u/n" (an escaped string on every fifth row, no such field elsewhere, an invalid
    document every thousandth) and "/id" (numbers, one string at row 3), the select twin's records uploaded and the real
    chain's, layout-only and with bytes: the whole arrays are the twin's, and every row is the reference's value
    (scale_selected).  The rows around index 262 144, where the second chunk begins, by name."""
    x = scale()
    check_scale_input(x)
    D = x.w.D
    assert (D + ROW_BLOCK - 1) // ROW_BLOCK == 1030 > SCAN_BLOCKS and D < ROW_GRID
    selected, out = scale_selected()
    ctwin = tcm.load_twin()
    a, d_sel, d_fields = device_select_fields(env, x, SCALE_PATHS, D + 37)
    d_buf = tvd.upload(env.dev, x.data)
    edge = SCAN_BLOCKS * ROW_BLOCK
    for p, pointer in ((1, "/u/n"), (0, "/id")):
        assert SCALE_PATHS[p] == pointer
        records = selected.column(p)[:D].copy()
        values = [out[(p, k)] for k in range(D)]
        up_fields, up_sel = tsc.upload_records(env.dev, records)
        for layout_only in (True, False):
            want = tcm.twin_column(ctwin, x.data, records, D, layout_only=layout_only)
            tcm.check_against_definition(want, values, records)
            tsc.same(tsc.device_column(env.dev, d_buf, len(x.data), up_fields, 0, up_sel, want), want, (pointer, "uploaded", layout_only))
            tsc.same(tsc.device_column(env.dev, a.d_buf, len(x.data), d_fields, p, d_sel, want), want, (pointer, "chain", layout_only))
        rows = want.rows()
        if pointer == "/u/n":
            assert want.res.n_strings == want.res.n_escaped == len(range(0, D, 5)) and want.res.n_other == 0
            assert rows[edge - 4:edge + 2] == [b"x\n%d" % (edge - 4), None, None, None, None, b"x\n%d" % (edge + 1)]
            assert int(want.offsets[edge]) == int(want.offsets[edge + 1]) == sum(len(b"x\n%d" % k) for k in range(0, edge, 5))
        else:
            assert rows[:5] == [None, None, None, b"dup", None] and rows[edge - 1:edge + 2] == [None] * 3
            assert (want.res.n_strings, want.res.total_bytes, want.res.n_other) == (1, 3, D - 1 - int(x.res.n_invalid))
            assert want.offsets[4:D + 1].tolist() == [3] * (D - 3)


WRAP_ROWS = ROW_GRID + 300
WRAP_PAST = 789                    # k % 1001 of the rows whose span runs past len: (ROW_GRID + 260) % 1001, and no multiple of 11 or 13
WRAP_UNIT = b"ab\\n\\u00e9cd\\ud83d\\ude00\\\\e"   # an escaped row names 1 .. 3 of these from a unit's first byte: 13 bytes (9 characters) each in the output


@functools.lru_cache(maxsize=None)
def wrap_records():
    """-> (data, length, records, long_at): WRAP_ROWS hand-made records over a buffer of some 80 KB: plain spans of 0 .. 40
    bytes cycling; an escaped short span every 11th; a record that is no string (a number's tag, or a code) every 13th; a
    span past `length` every 1 001st, at k % 1001 == WRAP_PAST -- 1 001 = 7 x 11 x 13, so at a multiple of 1 001 the record
    would be no string anyway; at this residue (no multiple of 11 or 13 either) it is a string's but for its span, every
    third of them flagged escaped, and they end past `length` and start past it in turn; 300 empty rows across index ROW_GRID; one plain row of 70 000 bytes and one
    long escaped row (a body of tests/escape_phases.py) in the second trip.  `length` is 1 000 bytes short of the buffer."""
    plain = b"abcdefghijklmnopqrstuvwxyz0123456789" * 100
    units = WRAP_UNIT * 40
    big = (b"0123456789 plain row " * 3400)[:70000]
    body = ep.body_of(ep.CARRIED + 61, ep.ESCAPES["pair_twice"], 333)
    data = plain + units + big + body + b"#" * 1200
    length = len(data) - 1000
    E0, P0, L0 = len(plain), len(plain) + len(units), len(plain) + len(units) + len(big)
    k = np.arange(WRAP_ROWS, dtype=np.int64)
    b, r = (k * 7) % (len(plain) - 41), k % 41
    typ, flags, code = np.full(WRAP_ROWS, ord('"'), dtype=np.uint8), np.zeros(WRAP_ROWS, dtype=np.uint8), np.zeros(WRAP_ROWS, dtype=np.uint16)
    esc = k % 11 == 0
    b, r = np.where(esc, E0 + ((k // 11) % 30) * len(WRAP_UNIT), b), np.where(esc, (1 + (k // 11) % 3) * len(WRAP_UNIT), r)
    flags[esc] = tcm.ESCAPED
    other, coded = k % 26 == 0, k % 26 == 13
    typ[other], typ[coded], code[coded] = ord("l"), 0, 20
    flags[other | coded] = 0
    past = k % 1001 == WRAP_PAST
    b, r = np.where(past, np.where((k // 1001) % 2 == 0, length - 5, length + 3), b), np.where(past, 10, r)
    flags[past & ((k // 1001) % 3 == 0)] = tcm.ESCAPED
    run = (k >= ROW_GRID - 150) & (k < ROW_GRID + 150)
    b, r = np.where(run, 5 + k % 100, b), np.where(run, 0, r)
    typ[run], flags[run], code[run] = ord('"'), 0, 0
    long_at = (ROW_GRID + 200, ROW_GRID + 230)
    b[long_at[0]], r[long_at[0]], b[long_at[1]], r[long_at[1]] = P0, len(big), L0, len(body)
    typ[list(long_at)], flags[list(long_at)], code[list(long_at)] = ord('"'), (0, tcm.ESCAPED), 0
    records = np.zeros(WRAP_ROWS, dtype=tsm.FIELD_DTYPE)
    records["bits"], records["type"], records["flags"], records["code"] = b.astype(np.uint64) | (r.astype(np.uint64) << np.uint64(32)), typ, flags, code
    return data, length, records, long_at


def restated_column(data, length, records):
    """The definition of the column in numpy, from the records alone: a row is a string when its record has no code, the
    string's tag and a span inside `length`; its bytes are its span's, unescaped (tests/tape_reference.py) when the record
    says escaped; offsets are the running sum of the valid rows' lengths, the bytes their concatenation
    -> (offsets, valid, bytes)"""
    b = (records["bits"] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    r = (records["bits"] >> np.uint64(32)).astype(np.int64)
    valid = (records["code"] == 0) & (records["type"] == ord('"')) & (b + r <= length)
    escaped = valid & ((records["flags"] & tcm.ESCAPED) != 0)
    pool, at = [np.frombuffer(data, dtype=np.uint8)], len(data)
    src, size = np.where(valid, b, 0), np.where(valid, r, 0)
    spans = {}
    for j in np.nonzero(escaped)[0].tolist():   # (a few dozen distinct spans, named over and over)
        key = (int(b[j]), int(r[j]))
        if key not in spans:
            out = tape_reference.unescape(b'"' + data[key[0]:key[0] + key[1]] + b'"', 0)
            spans[key] = (at, len(out))
            pool.append(np.frombuffer(out, dtype=np.uint8))
            at += len(out)
        src[j], size[j] = spans[key]
    offsets = np.concatenate([[0], np.cumsum(size)])
    pool = np.concatenate(pool)
    take = np.repeat(src - offsets[:-1], size) + np.arange(int(offsets[-1]), dtype=np.int64)
    return offsets.astype(np.uint64), valid.astype(np.uint8), pool[take]


def check_restated(col, data, length, records):
    offsets, valid, out = restated_column(data, length, records)
    D = len(records)
    assert np.array_equal(col.offsets[:D + 1], offsets) and np.array_equal(col.valid[:D], valid)
    assert (col.res.code, col.res.n_rows, col.res.n_strings, col.res.total_bytes) == (0, D, int(valid.sum()), out.size)
    assert col.res.n_other == int(((records["code"] == 0) & (valid == 0)).sum())
    assert col.res.n_escaped == int(((valid == 1) & ((records["flags"] & tcm.ESCAPED) != 0)).sum())
    if col.data is not None:
        assert np.array_equal(col.data[:out.size], out)
    assert col.untouched(D, out.size)
    return out.size


@pytest.mark.gpu
def test_string_column_grid_wrap(env):
    """More rows than sc_lengths / sc_copy reach in one trip of `v += gridDim.x` (4 096 blocks of 256 rows), and 4 098 block
    sums for sc_scan: hand-made records, uploaded.  The whole arrays are the twin's, layout-only and with bytes, and the
    twin's are the definition's restated in numpy.  With bytes_capacity one short: MSJ_CAPACITY, the true total, nothing
    written behind the capacity."""
    data, length, records, long_at = wrap_records()
    R = len(records)
    assert R == WRAP_ROWS > ROW_GRID and min(long_at) > ROW_GRID and length + 1000 == len(data)
    r = (records["bits"] >> np.uint64(32)).astype(np.int64)
    assert int(r[long_at[0]]) == 70000 and int(r[long_at[1]]) > LANE_BODY and int(records["flags"][long_at[1]]) == tcm.ESCAPED
    assert bool((r[ROW_GRID - 150:ROW_GRID + 150] == 0).all()) and int((records["code"] != 0).sum()) > R // 30
    # rows that are no strings through their span alone: a string's record without a code, plain and escaped, in both trips
    b = (records["bits"] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    by_span = (records["code"] == 0) & (records["type"] == ord('"')) & (b + r > length)
    named = ROW_GRID + 260
    assert named % 1001 == WRAP_PAST and bool(by_span[named]) and int(by_span.sum()) > 900
    assert int(records["flags"][named]) == tcm.ESCAPED and int((by_span & ((records["flags"] & tcm.ESCAPED) != 0)).sum()) > 300 and int((by_span & (b > length)).sum()) > 400
    assert int(by_span[:ROW_GRID].sum()) > 900 and bool((b[by_span] + r[by_span] <= len(data)).all())
    ctwin = tcm.load_twin()
    d_buf = tvd.upload(env.dev, data)
    d_fields, d_sel = tsc.upload_records(env.dev, records)
    for layout_only in (True, False):
        want = tcm.twin_column(ctwin, data, records, R, length=length, layout_only=layout_only)
        total = check_restated(want, data, length, records)
        tsc.same(tsc.device_column(env.dev, d_buf, length, d_fields, 0, d_sel, want), want, layout_only)
    rows = want.rows()
    assert rows[long_at[0]] == data[3600 + 40 * len(WRAP_UNIT):][:70000] and rows[ROW_GRID] == b"" and rows[1001] is None
    assert rows[named] is None and rows[named - 1] is not None and all(rows[j] is None for j in np.nonzero(by_span)[0].tolist())
    assert want.res.n_other == int(by_span.sum()) + int((records["type"] == ord("l")).sum())
    assert rows[long_at[1]] == b"x" * (ep.CARRIED + 61) + "\U0001F600\U0001F600".encode() + b"y" * 333
    assert rows[11] == b"ab\n\xc3\xa9cd\xf0\x9f\x98\x80\\e" * 2 and rows[R - 1] == data[int(records["bits"][R - 1]) & 0xFFFFFFFF:][:(R - 1) % 41]
    short = tcm.twin_column(ctwin, data, records, R, length=length, bytes_capacity=total - 1)
    tsc.same(tsc.device_column(env.dev, d_buf, length, d_fields, 0, d_sel, short), short, "one short")
    assert (short.res.code, short.res.total_bytes) == (MSJ_CAPACITY, total) and short.untouched(R, total - 1)
    assert np.array_equal(short.offsets, want.offsets) and np.array_equal(short.data[:total - 1], want.data[:total - 1])


@pytest.mark.gpu
def test_string_column_block_of_long_rows(env):
    """256 + 70 records across a block border that ALL name long escaped spans -- five bodies of 1 025 .. 5 000 raw bytes with
    their escapes at odd phases (tests/escape_phases.py), each named some 65 times, so every lane of every wave of the first
    block waits its turn in the ballot loop of sc_lengths / sc_copy, and the same span is walked again and again: the whole
    arrays are the twin's, and every row is Python's."""
    bodies = [ep.body_of(63, ep.ESCAPES["pair"], 950), ep.body_of(ep.CARRIED + 57, ep.ESCAPES["pair_twice"], 83),
              ep.body_of(61, ep.ESCAPES["five_n"], 2400), ep.body_of(ep.CARRIED + 59, ep.ESCAPES["u20ac_twice"], 2900),
              ep.body_of(4801, ep.ESCAPES["u00e9"], 193)]
    assert [len(x) for x in bodies] == [1025, 1252, 2467, 4059, 5000]
    data, starts = b"", []
    for body in bodies:
        starts.append(len(data) + 1)
        data += b'"' + body + b'"'
    R = ROW_BLOCK + 70
    records = np.concatenate([tcm.record(starts[k % 5], len(bodies[k % 5]), flags=tcm.ESCAPED) for k in range(R)])
    ctwin = tcm.load_twin()
    assert all(ctwin.scm_is_long(records[k:k + 1].ctypes.data, len(data), LANE_BODY) == 1 for k in range(R))
    d_buf = tvd.upload(env.dev, data)
    d_fields, d_sel = tsc.upload_records(env.dev, records)
    texts = [json.loads(b'"' + body + b'"').encode("utf-8") for body in bodies]
    for layout_only in (True, False):
        want = tcm.twin_column(ctwin, data, records, R, layout_only=layout_only)
        assert (want.res.code, want.res.n_strings, want.res.n_escaped) == (0, R, R)
        assert want.offsets[:R + 1].tolist() == [sum(len(texts[j % 5]) for j in range(k)) for k in range(R + 1)]
        tsc.same(tsc.device_column(env.dev, d_buf, len(data), d_fields, 0, d_sel, want), want, layout_only)
    assert want.rows() == [texts[k % 5] for k in range(R)]


ARRAY_LINES = DOC_GRID + 700


def array_line(k):
    """Line k of the array window: [] inside the run of 600 rows across DOC_GRID; every 1 000th, at offset 11, invalid;
    every 9th without "a"; every 7th an "a" that is no array; else k % 4 elements, numbers and short strings (every third
    string escaped)"""
    if DOC_GRID - 300 <= k < DOC_GRID + 300:
        return b'{"a":[]}'
    if k % 1000 == 11:
        return b'{"a":[1,tru]}'
    if k % 9 == 0:
        return b'{"b":%d}' % k
    if k % 7 == 0:
        return (b'{"a":%d}' % k, b'{"a":"s%d"}' % k, b'{"a":{"a":[%d]}}' % k)[k % 3]
    elements = [b"%d" % (k + j) if (k + j) % 2 else (b'"e\\n%d"' % k if (k + j) % 3 == 0 else b'"s%d"' % (k + j)) for j in range(k % 4)]
    return b'{"a":[' + b",".join(elements) + b"]}"


@functools.lru_cache(maxsize=None)
def array_window():
    """-> (Expected, select twin's Selected for "/a" with the verdicts given, {(0, k): (code, value)} held against the reference)"""
    lines = [array_line(k) for k in range(ARRAY_LINES)]
    x = Expected(b"\n".join(lines) + b"\n", lines)
    selected = tsm.twin_select(tsm.load_twin(), x.w, ["/a"], verdicts=x.rows)
    return x, selected, tsm.check_against_reference(x.w, selected, ["/a"], lines, codes=x.codes)


@pytest.mark.gpu
def test_array_column_row_wrap(env):
    """More documents than ac_rows has lanes (row_grid_blocks: 1 024 blocks of 256), so its loop makes a second trip and
    block_counter_add adds a workgroup's counts once behind it; 600 rows without an element across index 262 144.  The select
    twin's records uploaded and the real chain's: offsets, validity, elements and both results are the twin's, whole arrays
    with canaries, the twin's are the definition's on every row, and n_arrays, n_other and n_elements are counted in numpy.
    Then msj_string_column_device over the elements (more than 262 144 of them): the strings of the definition."""
    x, selected, values = array_window()
    D = x.w.D
    assert D == ARRAY_LINES > DOC_GRID and len(x.data) < 8 << 20
    k = np.arange(D)
    run = (k >= DOC_GRID - 300) & (k < DOC_GRID + 300)
    invalid = ~run & (k % 1000 == 11)
    missing = ~run & ~invalid & (k % 9 == 0)
    other = ~run & ~invalid & ~missing & (k % 7 == 0)
    arrays = ~invalid & ~missing & ~other
    n_elements = int((k % 4)[arrays & ~run].sum())
    assert [c != 0 for c in x.codes] == invalid.tolist() and int(run.sum()) == 600
    records = selected.column(0)[:D].copy()
    vals = [values[(0, j)] for j in range(D)]
    atwin, ctwin = tac.load_twin(), tcm.load_twin()
    full = tac.twin_lists(atwin, x.w, records)
    _, valid, items = tac.check_against_definition(x.w, full, vals)
    assert valid == arrays.astype(int).tolist() and len(items) == n_elements > DOC_GRID
    assert (full.res.n_arrays, full.res.n_other, full.res.n_elements) == (int(arrays.sum()), int(other.sum()), n_elements)
    assert int(full.offsets[DOC_GRID - 300]) == int(full.offsets[DOC_GRID + 300]) and int(full.offsets[DOC_GRID + 302]) > int(full.offsets[DOC_GRID])
    for chain in (False, True):
        if chain:
            a, d_sel, d_fields = device_select_fields(env, x, ["/a"], D + 3)
        else:
            a = tsd.Uploaded(env.dev, x.w, x.rows)
            d_fields, d_sel = tacd.upload_records(env.dev, [records], D)
        lay = tac.twin_lists(atwin, x.w, records, layout_only=True)
        assert lay.summary() == full.summary()
        tacd.same(tacd.device_lists(a, d_fields, 0, d_sel, lay)[0], lay, (chain, "layout only"))
        got, d_el, d_esel = tacd.device_lists(a, d_fields, 0, d_sel, full)
        tacd.same(got, full, chain)
        # the string column over the elements
        col = tcm.twin_column(ctwin, x.data, full.elements[:n_elements], n_elements)
        tsc.same(tsc.device_column(env.dev, a.d_buf, len(x.data), d_el.unsqueeze(0), 0, d_esel, col), col, (chain, "strings"))
    assert col.rows() == [v.encode("utf-8") if isinstance(v, str) else None for v in items] and col.res.n_escaped > 10000
