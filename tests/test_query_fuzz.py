"""The whole query chain as a user drives it -- ``DocumentStream`` and every view of a ``Window`` -- over the documents of
tests/query_fuzz.py, against that file's plain-Python model: per seed at three window sizes, the smallest with first guesses
of one document, one number, sixteen tape words and sixteen string bytes, so that every repair path of the stream runs on
windows that also start off the 16-byte grid and also hold invalid documents.

What include/msj_stage1.h leaves unspecified and no comparison here reads: the tape and string bytes of a document with a
verdict code (msj_document_tape: "tape_words ... 0 when code != 0", "string_bytes ... 0 when code != 0": ``documents()`` gives
None for it), and msj_dictionary_result.max_probe ("a diagnostic; not a function of the input alone").  Nothing else is
left out of a comparison."""
import json
import struct

import pytest

from tests import query_fuzz as qf
from tests import stream_order as so

pytestmark = pytest.mark.gpu
POINTERS = qf.pointers()
HOWS = ["inner", "left", "semi", "anti"]


@pytest.fixture(scope="module")
def dev():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mojo_simdjson_amd.device import Stage1Device

    d = Stage1Device(0)
    yield d
    d.close()


def byte_rows(column):
    """(offsets, bytes, valid) on the device -> bytes or None per row; a row that is not valid is empty"""
    off, data, valid = column[0].cpu().tolist(), column[1].cpu().numpy().tobytes(), column[2].cpu().tolist()
    assert all(valid[k] or off[k] == off[k + 1] for k in range(len(valid)))
    return [data[off[k]:off[k + 1]] if valid[k] else None for k in range(len(valid))]


def int_rows(column):
    return list(zip(column[0].cpu().tolist(), column[1].cpu().tolist()))


def double_rows(column):
    import torch

    return [(struct.pack("<q", b), ok) for b, ok in zip(column[0].view(torch.int64).cpu().tolist(), column[1].cpu().tolist())]


def texts(values):
    return [v.decode("utf-8") for v in values]


def together(entries):
    specs, cast = [], {}
    for s, c in entries:
        specs += s
        cast.update(c or {})
    return specs, cast


def group_by(m, paths, by=None, cast=None, rows=None):
    """The model's ``stats(paths, by=by, cast=cast)`` over `rows` (default: the documents)"""
    cast = cast or {}
    columns = {p: qf.cast(m.at(p, rows), cast[p]) if p in cast else [qf.number_value(n) for n in m.at(p, rows)] for p in paths}
    keys = None if by is None else qf.dictionary(m.strings(m.at(by, rows)))[:2]
    return qf.canon(m.stats(columns, keys))


def check_views(win, m):
    """Every view by pointer -> what they gave, per document, for the comparison across window sizes"""
    import torch

    D = len(m)
    per_document = [[] for _ in range(D)]

    def same(got, want, what, of_the_window=False):
        """of_the_window: a numbering that starts with the window, which another window size gives differently"""
        assert len(got) == len(want) == D, what
        assert got == want, (what, [(k, got[k], want[k]) for k in range(D) if got[k] != want[k]][:3])
        for k in range(D if not of_the_window else 0):
            per_document[k].append(got[k])

    for pointer in POINTERS:
        nodes = m.at(pointer)
        same(qf.canon(win.values(pointer)), m.values(nodes), ("values", pointer))
        same(int_rows(win.number_column(pointer, torch.int64)), m.number_column(nodes, "l"), ("int64", pointer))
        same(double_rows(win.number_column(pointer, torch.float64)), m.number_column(nodes, "d"), ("float64", pointer))
        strings = m.strings(nodes)
        same(byte_rows(win.strings(pointer)), strings, ("strings", pointer))
        same(byte_rows(win.raw(pointer)), m.raw(nodes), ("raw", pointer))
        same(byte_rows(win.raw(pointer, compact=True)), m.raw(nodes, True), ("compact", pointer))
        cats = win.categories(pointer)
        codes, values, first = qf.dictionary(strings)
        same(cats.codes.cpu().tolist(), codes, ("codes", pointer), of_the_window=True)
        assert (cats.values(), cats.first.cpu().tolist()) == (texts(values), first), ("categories", pointer)
        for unit in ("s", "ns"):
            same(int_rows(win.timestamps(pointer, unit)), m.ints(qf.cast(nodes, ("timestamp", unit))), ("timestamps", unit, pointer))
        for keep in (True, False):
            numbers = qf.cast(nodes, "number", keep)
            same(double_rows(win.parsed_numbers(pointer, keep_numbers=keep)), m.doubles(numbers), ("parsed", keep, pointer))
            same(int_rows(win.parsed_numbers(pointer, torch.int64, keep)), m.ints(numbers), ("parsed int64", keep, pointer))
    return per_document


def check_containers(win, m, per_document):
    listed = lambda rows: [None if row is None else m.values(row) for row in rows]
    tags, items = m.elements(m.at("/tags")), m.elements(m.at("/items"))
    got = qf.canon(win.elements("/tags").to_python())
    assert got == listed(tags)
    column = win.elements("/items")
    assert qf.canon(column.to_python()) == listed(items)
    flat = [n for row in items for n in row or []]
    assert column.n_elements == len(flat)
    fields = column.select(so.ELEMENT_POINTERS)
    # (a field that is found and null, and one that is missing, differ: ``ElementFields.to_python`` leaves the missing out)
    structs = [("o", [(p, qf.canon(node.value())) for p in so.ELEMENT_POINTERS for node in m.at(p, [n]) if node is not None]) for n in flat]
    want, j = [], 0
    for row in items:
        want.append(None if row is None else structs[j:j + len(row)])
        j += len(row or [])
    assert qf.canon(fields.to_python()) == want
    for p in so.ELEMENT_POINTERS:
        assert qf.canon(fields.values(p)) == m.values(m.at(p, flat)), p
    assert qf.canon(fields.elements("/tags").to_python()) == listed(m.elements(m.at("/tags", flat)))
    entries = m.entries(m.at("/attrs"))
    maps = win.entries("/attrs")
    want = [None if row is None else qf.canon(qf.first_wins((k.value(), v.value()) for k, v in row)) for row in entries]
    got_maps = qf.canon(maps.to_python())
    assert got_maps == want
    assert byte_rows(maps.keys()) == [k.value().encode("utf-8") for row in entries for k, _ in row or []]
    assert maps.schema() == m.schema(entries)
    for k in range(len(m)):
        per_document[k] += [got[k], got_maps[k]]


def check_where(win, m):
    plain = together([w for w in qf.WHERE if w[1] is None])
    for specs, cast in qf.WHERE + [plain, together(qf.WHERE[-3:-1])]:
        for any_ in (False, True):
            sel = win.where(specs, any=any_, cast=cast)
            kept = m.where(specs, any_, cast)
            assert sel.rows.cpu().tolist() == kept, (specs, any_)
            assert sel.keep.cpu().tolist() == [k in set(kept) for k in range(len(m))]
            assert qf.canon(sel.values("/id")) == m.values([m.at("/id")[k] for k in kept])


def check_take(win, m):
    """``take`` by a dictionary's first rows: one document per distinct value; a number past the window: missing values"""
    import torch

    cats = win.categories("/status")
    past = torch.tensor([len(m) + 3], dtype=torch.int32, device=cats.first.device)
    taken = win.take(torch.cat([cats.first, past]))
    _, values, first = qf.dictionary(m.strings(m.at("/status")))
    assert taken.values("/status") == texts(values) + [None]
    assert qf.canon(taken.values("/id")) == m.values([m.at("/id")[k] for k in first]) + [None]


def check_stats(win, m, sel, kept):
    rows = [m.roots[k] for k in kept]
    assert qf.canon(win.stats(["/latency"]).to_python()) == group_by(m, ["/latency"])
    assert qf.canon(win.stats(["/latency"], by="/status").to_python()) == group_by(m, ["/latency"], "/status")
    cast = {"/price": "number"}
    assert qf.canon(win.stats(["/latency", "/price"], by="/status", cast=cast).to_python()) == group_by(m, ["/latency", "/price"], "/status", cast)
    assert qf.canon(sel.stats(["/latency"]).to_python()) == group_by(m, ["/latency"], rows=rows)
    assert qf.canon(sel.stats(["/latency", "/price"], by="/status", cast=cast).to_python()) == \
        group_by(m, ["/latency", "/price"], "/status", cast, rows)
    # a group per row of the list column /items
    items = m.elements(m.at("/items"))
    flat = [n for row in items for n in row or []]
    row_of = [k for k, row in enumerate(items) for _ in row or []]
    q = [qf.number_value(n) for n in m.at("/q", flat)]
    got = win.elements("/items").select(["/q"]).stats(["/q"], per_row=True).to_python()
    assert qf.canon(got) == qf.canon(m.stats({"/q": q}, (row_of, None), n_groups=len(m)))


def check_order(win, m, sel, kept):
    D = len(m)
    latency = [qf.number_value(n) for n in m.at("/latency")]
    ts = qf.cast(m.at("/ts"), ("timestamp", "ns"))
    strings = m.strings(m.at("/status"))
    for view, rows in ((win, None), (sel, kept)):
        # (the rows of an ordered selection are the window's document numbers)
        rows_of = lambda ordered: ordered.rows.cpu().tolist()
        N = D if rows is None else len(rows)
        for kw in [dict(), dict(descending=True), dict(values_only=True)] + [dict(limit=n) for n in (1, max(D // 2, 1), D + 5)]:
            assert rows_of(view.order_by("/latency", **kw)) == qf.order(latency, rows, **kw), (N, kw)
        got = view.order_by([("/status", "asc"), ("/latency", "desc")], cast={"/status": "string"})
        want = qf.order(qf.string_ranks(strings), qf.order(latency, rows, descending=True))
        assert rows_of(got) == want
        assert qf.canon(got.values("/id")) == m.values([m.at("/id")[k] for k in want])
        assert rows_of(view.order_by("/ts", cast={"/ts": ("timestamp", "ns")})) == qf.order(ts, rows)


def check_join(win, m):
    strings, ids = m.strings(m.at("/status")), m.values(m.at("/id"))
    for how in HOWS:
        joined = win.join(win, "/status", how=how, by="string")
        want = qf.join(strings, strings, how)
        assert joined.left_rows.cpu().tolist() == [l for l, _ in want]
        with_right = how in ("inner", "left")
        if with_right:
            assert joined.right_rows.cpu().tolist() == [-1 if r is None else r for _, r in want]
        got = [(qf.canon(l), None if r is None else qf.canon(r)) for l, r in joined.to_python(["/id"], ["/id"])]
        assert got == [([ids[l]], [None if r is None else ids[r]] if with_right else None) for l, r in want], how


def run(dev, seed, window, tiny):
    """One pass of the stream over the seed's documents -> (what every document gave, the windows' facts)"""
    from mojo_simdjson_amd.document_stream import DocumentStream, RunningDictionary
    from tests import test_validate_documents as tvd

    lines, data = qf.lines(seed, qf.DOCUMENTS), qf.stream(seed, qf.DOCUMENTS)
    guesses = dict(documents=1, numbers=1, tape_words=16, string_bytes=16) if tiny else {}
    stream = DocumentStream(dev, tvd.upload(dev, data), len(data), window=window, select=POINTERS, parse=True, **guesses)
    sizes = lambda: (min(stream._doc_tapes.shape[0], stream._fields.shape[1]), stream._numbers.shape[0], stream._tape.shape[0], stream._sbuf.shape[0])
    before = sizes()
    rd = RunningDictionary(dev, dict_capacity=2, bytes_capacity=16)
    seen, windows, off_grid, per_document, codes = 0, 0, 0, [], []
    for win in stream:
        D = win.n_documents
        m = qf.Model(lines[seen:seen + D])
        assert D == len(m) and D > 0
        off_grid += win.base < win.document_offsets()[0]
        # the verdicts: how many, and which
        assert win.n_invalid == len(m.invalid)
        assert [k for k, c in enumerate((win.d_verdicts[:, 0] & 0xFFFFFFFF).cpu().tolist()) if c] == m.invalid
        assert win.first_invalid == (m.invalid[0] if m.invalid else None)
        documents = win.documents()
        assert [None if d is None else qf.canon(d.to_python()) for d in documents] == \
            [None if r is None else qf.canon(json.loads(r.text)) for r in m.roots]      # (``Document.to_python``: the last duplicate wins)
        rows = check_views(win, m)
        check_containers(win, m, rows)
        check_where(win, m)
        kept = m.where(qf.SELECTION[0])
        sel = win.where(qf.SELECTION[0])
        assert sel.rows.cpu().tolist() == kept
        check_stats(win, m, sel, kept)
        check_order(win, m, sel, kept)
        check_join(win, m)
        check_take(win, m)
        codes += win.categories("/status", dictionary=rd).codes.cpu().tolist()
        per_document += rows
        seen += D
        windows += 1
    assert seen == len(lines)
    whole = qf.Model(lines)
    want_codes, values, _ = qf.dictionary(whole.strings(whole.at("/status")))
    assert (codes, rd.values()) == (want_codes, texts(values))
    assert rd.order().values() == texts(sorted(values))
    return per_document, windows, off_grid, before, sizes()


SIZES = {"smallest": None, "4096": 4096, "1 << 20": 1 << 20}
RESULTS = {}    # {seed: {size: what every document gave}}: a case compares its own with those of the sizes that ran before it


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("seed", qf.SEEDS)
def test_the_chain_against_the_model(dev, seed, size):
    longest = max(len(t) for t, _ in qf.lines(seed, qf.DOCUMENTS))
    smallest = (longest + 32 + 15) // 16 * 16
    assert smallest <= 4096        # (else the middle size would have to go: the generator keeps its documents below that)
    window = SIZES[size] or smallest
    per_document, windows, off_grid, before, after = run(dev, seed, window, tiny=size == "smallest")
    if window < 1 << 20:
        assert windows >= 3 and off_grid >= 1
    else:
        assert windows == 1
    if size == "smallest":
        # documents, numbers, tape and string buffer each started too small and grew
        assert before == (1, 1, 16, 16) and all(a > b for a, b in zip(after, before)), (before, after)
    others = RESULTS.setdefault(seed, {})
    for name, other in others.items():
        assert per_document == other, name
    others[size] = per_document
