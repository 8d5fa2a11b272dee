"""``order_by`` with the cast "string" end to end (mojo_simdjson_amd/document_stream.py): a small NDJSON corpus on the device,
ordered by a string column through ``strings``, ``msj_dictionary_device``, msj_dictionary_order_device,
msj_rank_rows_device and msj_sort_rows_device.  The yardstick is ``json.loads`` over the file and ``sorted`` over the UTF-8
bytes of the values, rows without a string last in file order; ``RunningDictionary.order`` across three windows is held
against the order of the concatenated column."""
import json

import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mojo_simdjson_amd.device import Stage1Device

    d = Stage1Device(0)
    yield d
    d.close()


def ndjson(docs):
    return b"\n".join(json.dumps(d, ensure_ascii=False).encode() for d in docs) + b"\n"


def windows_of(dev, docs, select, window=1 << 20):
    from mojo_simdjson_amd.document_stream import DocumentStream
    from tests import test_validate_documents as tvd

    data = ndjson(docs)
    return iter(DocumentStream(dev, tvd.upload(dev, data), len(data), window=window, select=select))


NAMES = ["web-%02d" % (k * 7 % 31) for k in range(40)] + ["", "web", "web-", "Web-01", "zulu", "émile", "eve", "web-10.internal.example.org",
                                                          "web-10.internal.example.com", "web-10.internal.example.org/a", "日本", "a\u0000b", "a"]


def corpus():
    docs = [{"name": NAMES[k * 11 % len(NAMES)], "status": ("ok", "error", "timeout", "Ok")[k % 4], "latency_ms": (k * 37) % 101, "n": k} for k in range(400)]
    docs[3] = {"status": "ok", "latency_ms": 5, "n": 3}            # no name
    docs[8] = {"name": 8, "status": None, "latency_ms": 1.5, "n": 8}   # not strings
    docs[21] = {"name": None, "status": "ok", "n": 21}
    return docs


def text(doc, key):
    v = doc.get(key)
    return v.encode() if isinstance(v, str) else None


def py_order(docs, key, descending=False, values_only=False, rows=None):
    """The row numbers by the key's bytes, stable, rows without a string last (or left out)"""
    rows = list(range(len(docs))) if rows is None else rows
    have = [k for k in rows if text(docs[k], key) is not None]
    have.sort(key=lambda k: text(docs[k], key), reverse=descending)   # (stable in both directions: equal values keep input order)
    return have + ([] if values_only else [k for k in rows if text(docs[k], key) is None])


def test_order_by_a_string_column(dev):
    docs = corpus()
    win = next(windows_of(dev, docs, ["/name", "/status", "/latency_ms", "/n"]))
    cast = {"/name": "string"}
    assert win.order_by("/name", cast=cast).rows.cpu().tolist() == py_order(docs, "name")
    assert win.order_by("/name", cast=cast, descending=True).rows.cpu().tolist() == py_order(docs, "name", descending=True)
    assert win.order_by("/name", cast=cast, limit=10).rows.cpu().tolist() == py_order(docs, "name")[:10]
    assert win.order_by("/name", cast=cast, values_only=True).rows.cpu().tolist() == py_order(docs, "name", values_only=True)
    first = win.order_by("/name", cast=cast, limit=7)
    assert first.values("/n") == [docs[k]["n"] for k in py_order(docs, "name")[:7]]
    with pytest.raises(ValueError):
        win.where([("/name", "==", "web")], cast={"/name": "string"})
    with pytest.raises(ValueError):
        win.stats(["/latency_ms"], cast={"/latency_ms": "string"})


def test_two_keys_a_string_and_a_number(dev):
    docs = corpus()
    win = next(windows_of(dev, docs, ["/name", "/status", "/latency_ms", "/n"]))
    got = win.order_by([("/status", "asc"), ("/latency_ms", "desc")], cast={"/status": "string"}).rows.cpu().tolist()
    number = lambda k: docs[k].get("latency_ms") if isinstance(docs[k].get("latency_ms"), (int, float)) else None
    minor = sorted([k for k in range(len(docs)) if number(k) is not None], key=lambda k: -number(k)) + [k for k in range(len(docs)) if number(k) is None]
    assert got == py_order(docs, "status", rows=minor)


def test_a_row_selection_and_list_elements(dev):
    docs = corpus()
    win = next(windows_of(dev, docs, ["/name", "/status", "/latency_ms", "/n"]))
    sel = win.where([("/latency_ms", "<", 50)])
    kept = [k for k in range(len(docs)) if isinstance(docs[k].get("latency_ms"), (int, float)) and docs[k]["latency_ms"] < 50]
    assert sel.rows.cpu().tolist() == kept
    got = sel.order_by("/name", cast={"/name": "string"}, limit=25)
    want = py_order(docs, "name", rows=kept)[:25]   # (the rows of an ordered selection are the window's document numbers)
    assert got.rows.cpu().tolist() == want and got.values("/n") == [docs[k]["n"] for k in want]
    lists = [{"tags": ["b", "a", "", "ab", 3, "a", None, "B"]}, {"tags": []}, {"tags": ["zz", "aé"]}]
    lwin = next(windows_of(dev, lists, ["/tags"]))
    elements = [t for d in lists for t in d["tags"]]
    order, _ = lwin.elements("/tags").order(cast="string")
    flat = [{"t": t} for t in elements]
    assert order.cpu().tolist() == py_order(flat, "t")


def test_dictionary_order_of_a_column_and_across_windows(dev):
    from mojo_simdjson_amd.document_stream import DictionaryOrder, RunningDictionary

    docs = corpus()
    win = next(windows_of(dev, docs, ["/name"]))
    cat = win.categories("/name")
    order = cat.order()
    names = [d["name"] for d in docs if isinstance(d.get("name"), str)]
    assert isinstance(order, DictionaryOrder) and order.result.code == 0 and order.result.n_equal == 0
    assert order.values() == [b.decode() for b in sorted(set(n.encode() for n in names))]
    assert order.sorted[order.rank.long()].cpu().tolist() == list(range(cat.n_distinct))
    records, _ = order.rank_records(cat.codes)
    ranks = {v: r for r, v in enumerate(order.values())}
    assert [None if code else bits for bits, code in zip(records[:, 0].cpu().tolist(), (records[:, 1] >> 48).cpu().tolist())] == \
        [ranks.get(d.get("name")) if isinstance(d.get("name"), str) else None for d in docs]
    # one call of one round leaves the long shared prefixes tied: the wrapper continues it to the same order
    short = cat.order(max_rounds=1)
    assert short.result.code == 0 and short.result.depth > 8 and short.sorted.cpu().tolist() == order.sorted.cpu().tolist()
    # a running dictionary over three windows: the order of the concatenated column
    rd = RunningDictionary(dev, dict_capacity=4, bytes_capacity=16)
    codes, windows = [], 0
    for w in windows_of(dev, docs, ["/name"], window=8192):
        codes += w.categories("/name", dictionary=rd).codes.cpu().tolist()
        windows += 1
    assert windows >= 3 and len(codes) == len(docs)
    whole = rd.order()
    assert whole.values() == order.values() and whole.n_entries == rd.n_distinct
    rank = whole.rank.cpu().tolist()
    by_rank = sorted(range(len(docs)), key=lambda k: (codes[k] < 0, rank[codes[k]] if codes[k] >= 0 else 0, k))
    assert by_rank == py_order(docs, "name")
