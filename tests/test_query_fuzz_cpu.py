"""tests/query_fuzz.py on a machine without a GPU: the generator keeps its own conditions, and the model equals the host twins
-- the chain of tests/stream_order.py over the generated stream, then the twins of the row calls over that chain's select
records.  A twin compiles the ``csrc/*_math.h`` its kernel compiles, the model is plain Python written from the header's
prose: an error of meaning in a shared header shows here."""
import collections
import functools
import json

import numpy as np
import pytest
import torch

from mojo_simdjson_amd import _lib
from mojo_simdjson_amd.document_stream import FIELD_DTYPE, GroupStats, field_value
from tests import query_fuzz as qf
from tests import stream_order as so
from tests import test_aggregate_math as tam
from tests import test_cast_strings_math as tcs
from tests import test_dictionary_order_math as tdo
from tests import test_filter_rows_math as tfm
from tests import test_join_rows_math as tjm
from tests import test_select_math as tsm
from tests import test_sort_rows_math as tsr
from tests import test_string_column_math as tcm

POINTERS = qf.pointers()
SEEDS = qf.SEEDS


class Fuzz:
    """One seed: the generator's lines, the stream, the twins' chain over it, the model"""

    def __init__(self, seed):
        self.g = qf.generate(seed, qf.DOCUMENTS)
        self.data = qf.stream(seed, qf.DOCUMENTS)
        assert self.data.endswith(b"\n")                           # (the last separator; so.Expected puts it back)
        self.e = so.Expected.from_lines("fuzz-%d" % seed, [self.data[:-1]])
        assert self.e.data == self.data
        self.m = qf.Model(self.g.lines)
        e, w = self.e, self.e.w
        self.D = w.D
        self.sel = tsm.twin_select(so.twins().s, w, POINTERS, verdicts=e.verdicts, capacity=w.D)
        self.host = (np.frombuffer(e.data, dtype=np.uint8), w.idx, w.end)

    def column(self, pointer):
        return self.sel.column(POINTERS.index(pointer))[:self.D]

    def decoded(self, records):
        return [None if r["code"] else qf.canon(field_value(r, *self.host)) for r in records]


@functools.lru_cache(maxsize=None)
def fuzz(seed):
    return Fuzz(seed)


# ---- the generator's conditions ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", SEEDS)
def test_generator_conditions(seed):
    g = qf.generate(seed, qf.DOCUMENTS)
    n_bad = sum(kind is not None for kind in g.kinds)
    assert 0.05 * qf.DOCUMENTS <= n_bad <= 0.15 * qf.DOCUMENTS
    for (text, doc), kind in zip(g.lines, g.kinds):
        assert (doc is qf.INVALID) == (kind is not None)
        assert b"\x00" not in text and not any(c < 0x20 and c not in b"\t\n\r" for c in text)     # no raw control character
        if kind is None:
            got = json.loads(text, object_pairs_hook=qf.first_wins, parse_constant=qf.refuse_constant)
            assert qf.canon(got) == qf.canon(doc) and not qf.array_too_deep(got, 0, qf.MAX_DEPTH)
        elif kind == "depth":
            assert qf.array_too_deep(json.loads(text), 0, qf.MAX_DEPTH) and not qf.array_too_deep(json.loads(text), 0, qf.MAX_DEPTH + 1)
        elif kind == "1e400":
            assert b"1e400" in text and qf.cast_number(b"1e400") is None and qf.cast_number(b"1e308") == 1e308
        else:
            assert qf.python_rejects(text), (kind, text)
    # the sum bound: every summed number on the grid (the generator asserts it where it draws them; here over what it wrote)
    m = qf.Model(g.lines)
    summed = [qf.number_value(n) for n in m.at("/latency")] + qf.cast(m.at("/price"), "number")
    summed += [qf.number_value(n) for row in qf.Model.elements(m.at("/items")) for n in m.at("/q", row or [])]
    for v in summed:
        if v is not None:
            qf.summable(repr(v))


def test_every_feature_occurs():
    total = collections.Counter()
    for seed in SEEDS:
        total += qf.generate(seed, qf.DOCUMENTS).count
    wanted = ["style " + s for s in qf.STYLES] + ["separator none", "separator blank", "escaped key", "escaped slash", "surrogate pair",
                                                    "escaped non-ascii", "escaped ascii", "attrs empty key", "attrs duplicate key",
                                                    "duplicate behind the first", "duplicate before the first", "status no string",
                                                    "latency no number", "ts leap day", "ts other", "ts escaped", "ts no string", "ts offset Z",
                                                    "ts offset +", "ts offset -", "price number", "price other", "price escaped",
                                                    "price no string", "id number", "id other", "id escaped", "id no string", "tags empty",
                                                    "tags nested", "tags no list", "attrs no object", "item no object", "item duplicate key",
                                                    "items no list", "geo scalar", "root no object", "root deep"]
    wanted += ["ts fraction %d" % d for d in range(10)] + ["items %d" % n for n in range(5)] + ["invalid " + k for k in qf.INVALID_KINDS]
    wanted += ["status " + repr(s) for s in qf.STATUS] + ["latency " + t for t in qf.LATENCY] + ["unsummed " + t for t in qf.UNSUMMED]
    wanted += ["absent " + k for k in ("status", "tags", "attrs", "items", "geo", "latency", "ts", "price", "id")]
    assert {f: total[f] for f in wanted if total[f] < 3} == {}
    # the same status value arrives under different bytes
    texts = collections.defaultdict(set)
    for seed in SEEDS:
        m = qf.Model(qf.lines(seed, qf.DOCUMENTS))
        for node in m.at("/status"):
            if node is not None and node.tag == '"':
                texts[node.value()].add(node.text)
    assert all(len(texts[s]) >= 2 for s in qf.STATUS if s != "")


# ---- the model against the chain's twins ------------------------------------------------------------------------------------

def rows_of(column, D):
    off = column.offsets[:D + 1].tolist()
    return [bytes(column.data[off[k]:off[k + 1]]) if column.valid[k] else None for k in range(D)]


def lists_of(f, lists, rows):
    off = lists.offsets[:rows + 1].tolist()
    return [f.decoded(lists.elements[off[k]:off[k + 1]]) if lists.valid[k] else None for k in range(rows)]


@pytest.mark.parametrize("seed", SEEDS)
def test_model_against_the_chain(seed):
    f = fuzz(seed)
    e, m, D = f.e, f.m, f.D
    assert D == len(m)
    assert [k for k, c in enumerate(e.codes) if c] == m.invalid
    assert e.codes == [qf.INVALID_CODES[kind] if kind else 0 for kind in f.g.kinds]
    for pointer in POINTERS:
        assert f.decoded(f.column(pointer)) == m.values(m.at(pointer)), pointer
    assert rows_of(e.strings, D) == m.strings(m.at("/status"))
    for compacted in (False, True):
        assert rows_of(e.raw[compacted], D) == m.raw(m.at("/geo"), compacted)
    # the lists of /items, the fields of their elements, the lists of /items[*].tags
    items = m.elements(m.at("/items"))
    assert lists_of(f, e.lists, D) == [None if row is None else m.values(row) for row in items]
    flat = [n for row in items for n in row or []]
    assert e.E == len(flat)
    for p, pointer in enumerate(so.ELEMENT_POINTERS):
        assert f.decoded(e.efields.column(p)[:e.E]) == m.values(m.at(pointer, flat)), pointer
    sub = m.elements(m.at("/tags", flat))
    assert lists_of(f, e.sublists, e.E) == [None if row is None else m.values(row) for row in sub]
    # the map of /attrs: every entry, duplicates kept, in document order
    entries = m.entries(m.at("/attrs"))
    off = e.maps.offsets[:D + 1].tolist()
    got = [list(zip(f.decoded(e.maps.keys[off[k]:off[k + 1]]), f.decoded(e.maps.values[off[k]:off[k + 1]]))) if e.maps.valid[k] else None
           for k in range(D)]
    assert got == [None if row is None else list(zip(m.values([k for k, _ in row]), m.values([v for _, v in row]))) for row in entries]
    # the dictionaries: codes in the order of first appearance.  (max_probe is not compared: msj_dictionary_result, "the
    # longest probe sequence ... depends on the order of insertion")
    for encoded, strings in ((e.dict_strings, m.strings(m.at("/status"))), (e.dict_raw, m.raw(m.at("/geo"), True))):
        codes, values, first = qf.dictionary(strings)
        assert (encoded.codes[:D].tolist(), encoded.values(), encoded.dict_first[:len(values)].tolist()) == (codes, values, first)


# ---- the row calls' twins over the chain's records --------------------------------------------------------------------------

def numbers_of(records):
    return [tfm.number_of(r) for r in records]


def twin_cast(f, pointer, spec, keep_numbers=None):
    """The cast twin over a pointer's records -> the cast records"""
    kind, unit = (spec, "s") if isinstance(spec, str) else spec            # (a number has no unit: the call wants 0)
    keep = kind == "number" if keep_numbers is None else keep_numbers
    got = tcs.twin_cast(tcs.load_twin(), f.e.data, f.column(pointer), _lib.CAST_KINDS[kind], unit, _lib.CAST_KEEP_NUMBERS if keep else 0)
    assert got.rc == 0 and got.res.code == 0
    return got.records(f.D).copy()


@pytest.mark.parametrize("seed", SEEDS)
def test_cast_twin(seed):
    f = fuzz(seed)
    for pointer, spec in (("/ts", ("timestamp", "s")), ("/ts", ("timestamp", "ns")), ("/ts", ("timestamp", "ms")), ("/price", "number"),
                          ("/id", "number")):
        for keep in (False, True):
            got = numbers_of(twin_cast(f, pointer, spec, keep))
            assert qf.canon(got) == qf.canon(qf.cast(f.m.at(pointer), spec, keep)), (pointer, spec, keep)


def twin_specs(f, specs, cast):
    """``where``'s specs by pointer -> (tfm.Spec by column number, the columns, the string values per column)"""
    used = []

    def one(spec, neg=False):
        if len(spec) == 2 and spec[0] == "not":
            return one(spec[1], True)
        pointer, op = spec[0], spec[1]
        if pointer not in used:
            used.append(pointer)
        c, operand = used.index(pointer), spec[2] if len(spec) > 2 else None
        if op == "found":
            return tfm.Spec(c, tfm.FOUND, None, neg)
        if op == "type":
            names = [operand] if isinstance(operand, str) else operand
            mask = 0
            for name in names:
                for tag in qf.TYPE_TAGS[name]:
                    mask |= _lib.TYPE_BITS[tag]
            return tfm.Spec(c, tfm.TYPE, mask, neg)
        if isinstance(operand, str):
            return tfm.Spec(c, tfm.STR_EQ if op == "==" else tfm.STR_PREFIX, operand.encode("utf-8"), neg)
        if not isinstance(operand, (int, float)):
            operand = qf.datetime_units(operand, cast[pointer][1])
        return tfm.Spec(c, {"==": tfm.NUM_EQ, "<": tfm.NUM_LT, "<=": tfm.NUM_LE, ">": tfm.NUM_GT, ">=": tfm.NUM_GE}[op], operand, neg)

    out = [one(s) for s in specs]
    columns = [twin_cast(f, p, cast[p]) if cast and p in cast else f.column(p) for p in used]
    return out, np.concatenate(columns)


def twin_where(f, specs, any_, cast):
    ftwin = tfm.load_twin()
    compiled, fields = twin_specs(f, specs, cast)
    blob = tfm.compile_specs(ftwin, compiled, any_)
    got = tfm.twin_filter(ftwin, blob, f.e.data, len(f.e.data), fields, f.D, len(fields) // f.D, tcm.select_result(f.D), f.D)
    assert got.rc == 0 and got.res.code == 0 and got.res.n_rows == f.D
    kept = got.kept[:got.res.n_kept].tolist()
    assert [k for k in range(f.D) if got.keep[k]] == kept
    return kept


def together(entries):
    specs, cast = [], {}
    for s, c in entries:
        specs += s
        cast.update(c or {})
    return specs, cast


@pytest.mark.parametrize("seed", SEEDS)
def test_filter_twin(seed):
    f = fuzz(seed)
    plain = together([w for w in qf.WHERE if w[1] is None])
    assert len(plain[0]) == 16
    for specs, cast in qf.WHERE + [plain, together(qf.WHERE[-3:-1])]:
        for any_ in (False, True):
            assert twin_where(f, specs, any_, cast) == f.m.where(specs, any_, cast), (specs, any_)
    assert 0 < len(f.m.where(qf.SELECTION[0])) < f.D


def group_stats(columns, R, codes, G, names, labels):
    """The aggregate twin -> what ``GroupStats.to_python`` makes of its records"""
    got = tam.twin_aggregate(tam.load_twin(), columns, R, codes, G)
    assert got.rc == 0 and got.res.code == 0 and got.res.n_rows == R
    records = torch.from_numpy(np.ascontiguousarray(got.records(G)).view(np.uint8).reshape(len(names), G, 48).copy())
    out = GroupStats(None, names, records, got.res).to_python()
    for g, row in enumerate(out):
        if labels is not None:
            row = out[g] = {"key": labels[g].decode("utf-8"), **row}
    return qf.canon(out)


@pytest.mark.parametrize("seed", SEEDS)
def test_aggregate_twin(seed):
    f = fuzz(seed)
    m, D = f.m, f.D
    latency = [qf.number_value(n) for n in m.at("/latency")]
    assert group_stats(f.column("/latency"), D, None, 1, ["/latency"], None) == qf.canon(m.stats({"/latency": latency}))
    codes, values, _ = qf.dictionary(m.strings(m.at("/status")))
    assert len(values) == len(qf.STATUS)
    price = qf.cast(m.at("/price"), "number")
    columns = np.stack([f.column("/latency"), twin_cast(f, "/price", "number")])
    got = group_stats(columns, D, np.array(codes, dtype=np.int32), len(values), ["/latency", "/price"], values)
    assert got == qf.canon(m.stats({"/latency": latency, "/price": price}, (codes, values)))
    # on a selection: the rows taken
    kept = m.where(qf.SELECTION[0])
    want = m.stats({"/latency": [latency[k] for k in kept]}, ([codes[k] for k in kept], values))
    got = group_stats(f.column("/latency")[kept], len(kept), np.array(codes, dtype=np.int32)[kept], len(values), ["/latency"], values)
    assert got == qf.canon(want)
    # a group per row of the list column /items over the elements' /q
    items = m.elements(m.at("/items"))
    flat = [n for row in items for n in row or []]
    rows = [k for k, row in enumerate(items) for _ in row or []]
    q = [qf.number_value(n) for n in m.at("/q", flat)]
    got = group_stats(f.e.efields.column(so.ELEMENT_POINTERS.index("/q"))[:f.e.E], f.e.E, np.array(rows, dtype=np.int32), D, ["/q"], None)
    assert got == qf.canon(m.stats({"/q": q}, (rows, None), n_groups=D))
    # both the int and the double sum, the overflow flag, -0.0 and a group without a value occur
    seen = [r["/latency"] for r in m.stats({"/latency": latency}, (codes, values))]
    assert any(isinstance(r["sum"], float) for r in seen)


@pytest.mark.parametrize("seed", SEEDS[:2])
def test_numbers_without_bits(seed):
    """The select twin without number records: every number is an MSJ_FIELD_NO_BITS record, which is found and has its
    type, and has no number value for a compare, a sum or an order (msj_filter_rows_device, msj_aggregate_device "Number
    value", msj_sort_rows_device)"""
    f = fuzz(seed)
    m, D = f.m, f.D
    sel = tsm.twin_select(so.twins().s, f.e.w, ["/latency"], verdicts=f.e.verdicts, capacity=D, numbers=False)
    column = sel.column(0)[:D]
    numbers = [qf.number_value(n) is not None for n in m.at("/latency")]
    assert [bool(r["flags"] & _lib.FIELD_NO_BITS) for r in column] == numbers and sum(numbers) > D // 2
    ftwin = tfm.load_twin()
    for spec, want in ((tfm.Spec(0, tfm.NUM_GE, -(1 << 63)), []), (tfm.Spec(0, tfm.TYPE, 8 | 16), [k for k in range(D) if numbers[k]]),
                       (tfm.Spec(0, tfm.NUM_LT, 0.5, neg=True), list(range(D)))):
        got = tfm.twin_filter(ftwin, tfm.compile_specs(ftwin, [spec]), f.e.data, len(f.e.data), column, D, 1, tcm.select_result(D), D)
        assert got.kept[:got.res.n_kept].tolist() == want and got.res.n_no_bits == (sum(numbers) if spec.op != tfm.TYPE else 0)
    got = tam.twin_aggregate(tam.load_twin(), column, D, None, 1)
    assert (got.res.n_values, got.res.n_skipped) == (0, sum(numbers)) and int(got.records(1)[0, 0]["n_rows"]) == D
    got = tsr.twin_sort(tsr.load_twin(), column, D)
    assert got.rows() == list(range(D)) and got.counts() == (D, 0, D, sum(numbers), 0)
    assert tsr.twin_sort(tsr.load_twin(), column, D, flags=2).rows() == []


def twin_order(col, R, rows_in=None, descending=False, limit=None, values_only=False):
    got = tsr.twin_sort(tsr.load_twin(), col, R, rows_in, flags=int(descending) | 2 * int(values_only), limit=int(limit or 0))
    assert got.rc == 0 and got.res.code == 0
    return got.rows()


def rank_records(f, strings_column):
    """The twins of msj_dictionary_order_device and msj_rank_rows_device over a twin's dictionary -> the rank records"""
    tw = tdo.load_twin()
    d = tdo.Dict(strings_column.values())
    rc, res, srt, rnk, _ = tdo.run_twin(tw, d, max_rounds=64)
    assert rc == 0 and res.code == 0
    codes = np.ascontiguousarray(strings_column.codes[:f.D], dtype=np.int32)
    rc, rres, _, fields = tdo.run_rank_rows(tw, codes, rnk, res)
    assert rc == 0 and rres.code == 0
    return srt[:d.V].tolist(), fields.view(FIELD_DTYPE)


@pytest.mark.parametrize("seed", SEEDS)
def test_sort_twin(seed):
    f = fuzz(seed)
    m, D = f.m, f.D
    latency = [qf.number_value(n) for n in m.at("/latency")]
    kept = m.where(qf.SELECTION[0])
    for rows in (None, kept):
        N = D if rows is None else len(rows)
        for kw in [dict(), dict(descending=True), dict(values_only=True), dict(descending=True, values_only=True)] + \
                  [dict(limit=n) for n in (1, max(N // 2, 1), N + 5)]:
            assert twin_order(f.column("/latency"), D, rows, **kw) == qf.order(latency, rows, **kw), (rows is None, kw)
        ts = qf.cast(m.at("/ts"), ("timestamp", "ns"))
        assert twin_order(twin_cast(f, "/ts", ("timestamp", "ns")), D, rows) == qf.order(ts, rows)
        # two keys, the major one a string through its dictionary's order and the rows' ranks
        strings = m.strings(m.at("/status"))
        srt, ranks = rank_records(f, f.e.dict_strings)
        _, values, _ = qf.dictionary(strings)
        assert [values[c] for c in srt] == sorted(values)
        minor = twin_order(f.column("/latency"), D, rows, descending=True)
        assert twin_order(ranks, D, minor) == qf.order(qf.string_ranks(strings), qf.order(latency, rows, descending=True))


@pytest.mark.parametrize("seed", SEEDS)
def test_join_twin(seed):
    f = fuzz(seed)
    strings = f.m.strings(f.m.at("/status"))
    codes = np.ascontiguousarray(f.e.dict_strings.codes[:f.D], dtype=np.int32)
    G = int(f.e.dict_strings.res.n_distinct)
    for how, kind in _lib.JOIN_KINDS.items():
        got = tjm.twin_join(tjm.load_twin(), codes, codes, G, kind)
        assert got.rc == 0 and got.res.code == 0
        M = int(got.res.n_pairs)
        pairs = [(int(l), None if r == 0xFFFFFFFF else int(r)) for l, r in zip(got.left[:M], got.right[:M])]
        want = qf.join(strings, strings, how)
        if how == "anti":
            assert [r for _, r in pairs] == [None] * M
        assert pairs == want, how
