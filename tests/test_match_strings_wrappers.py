"""The substring operators of the where methods and ``match`` of the record views (mojo_simdjson_amd.document_stream over
msj_match_strings_device), against ``json.loads`` and Python's ``in`` / ``endswith`` / ``re`` on a small NDJSON corpus with
escaped values, non-string values, missing keys and a document with a verdict code.  The specs' rewriting is checked without
a device."""
import json
import re

import numpy as np
import pytest

from mojo_simdjson_amd.document_stream import _match_pattern, _match_specs
from tests import test_match_strings_math as tmm

gpu = pytest.mark.gpu


# ---- the specs, without a device ------------------------------------------------------------------------------------------------

def test_operands_become_patterns():
    assert _match_pattern("contains", "timeout") == ([b"timeout"], set())
    assert _match_pattern("icontains", b"a%_") == ([b"a%_"], {"nocase"})
    assert _match_pattern("suffix", ".png") == ([b".png"], {"at_end"})
    assert _match_pattern("isuffix", "é") == (["é".encode()], {"at_end", "nocase"})
    assert _match_pattern("like", "GET %.png") == ([b"GET ", b".png"], {"at_start", "at_end"})
    assert _match_pattern("like", "%a%b%") == ([b"a", b"b"], set())
    assert _match_pattern("like", "%a") == ([b"a"], {"at_end"})
    assert _match_pattern("like", "a%") == ([b"a"], {"at_start"})
    assert _match_pattern("ilike", "abc") == ([b"abc"], {"at_start", "at_end", "nocase"})
    assert _match_pattern("like", b"a%b%c%d") == ([b"a", b"b", b"c", b"d"], {"at_start", "at_end"})
    for op in ("==", "prefix", "found", "icontain", "i", "ilikes"):
        assert _match_pattern(op, "x") is None
    for op, operand in (("like", "a%%b"), ("like", "%"), ("like", "%%"), ("like", ""), ("like", "a_b"), ("ilike", "_"), ("contains", ""),
                        ("suffix", b""), ("contains", 5), ("like", None)):
        with pytest.raises(ValueError):
            _match_pattern(op, operand)


def test_specs_are_rewritten_to_found():
    specs = [(1, "contains", "x"), ("not", (1, "like", "a%b")), (2, ">", 5), (0, "isuffix", "y"), ("not", ("not", (1, "==", "z")))]
    out, wanted = _match_specs(specs, 3)
    assert out == [(3, "found"), ("not", (4, "found")), (2, ">", 5), (5, "found"), ("not", ("not", (1, "==", "z")))]
    assert wanted == {1: [(3, ([b"x"], set())), (4, ([b"a", b"b"], {"at_start", "at_end"}))], 0: [(5, ([b"y"], {"at_end", "nocase"}))]}
    assert _match_specs([(0, "found"), (1, "==", "contains")], 2) == ([(0, "found"), (1, "==", "contains")], {})


# ---- on the device --------------------------------------------------------------------------------------------------------------

WORDS = ("timeout", "Timeout", "TIMEOUT after 5s", "connection reset", "ok", "", "read timeout: upstream", "time out", "a\"b", "x.png", "X.PNG",
         "GET /img/a.png", "get /IMG/b.PNG", "GET /img/a.png?x", "é timeout é", "100%", "a_b")


def make_lines():
    lines = []
    for k in range(240):
        doc = {"id": k, "latency": (k * 37) % 500, "price": "%d.5" % (k % 90), "status": ("ok", "error", "warn")[k % 3]}
        m = WORDS[(k * 7) % len(WORDS)] + (" #%d" % k if k % 4 == 0 else "")
        if k % 11 == 3:
            doc["message"] = (k, None, True, {"message": "timeout"}, ["timeout"])[k % 5]
        elif k % 13 != 5:
            doc["message"] = m
        doc["tags"] = [WORDS[(k + j) % len(WORDS)] if (k + j) % 5 else j for j in range(k % 4)] if k % 6 else "timeout"
        doc["items"] = [{"name": WORDS[(k * 3 + j) % len(WORDS)], "qty": j} if (k + j) % 7 else {"qty": "timeout"} for j in range(k % 3)]
        lines.append(json.dumps(doc, ensure_ascii=bool(k % 2)).encode())
    lines[10] = b'{"id":10,"latency":1,"price":"1.5","status":"ok","message":"\\u0074imeout \\u00e9","tags":[],"items":[]}'
    lines[20] = b'{"id":20,"latency":2,"price":"2.5","status":"ok","message":"a\\"b and \\ttab","tags":["a\\"b"],"items":[{"name":"\\u0078.png"}]}'
    lines[30] = b'{"id":30,"latency":3,"message":"timeout","status":"ok","tags":[tru],"items":[]}'  # a verdict code
    return lines


POINTERS = ["/message", "/status", "/latency", "/price", "/tags", "/items", ""]


@pytest.fixture(scope="module")
def env():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mojo_simdjson_amd.device import Stage1Device
    from mojo_simdjson_amd.document_stream import DocumentStream

    dev = Stage1Device(0)
    lines = make_lines()
    data = b"\n".join(lines) + b"\n"
    d_buf = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(dev.device)
    docs = [None if k == 30 else json.loads(line) for k, line in enumerate(lines)]

    class Env:
        pass

    e = Env()
    e.dev, e.lines, e.docs = dev, lines, docs
    e.stream = lambda window=8192: DocumentStream(dev, d_buf, len(data), window=window, select=POINTERS)
    yield e
    dev.close()


def text(doc, key="message"):
    v = None if doc is None else doc.get(key)
    return v.encode() if isinstance(v, str) else None


def like(pattern, v, nocase=False):
    rx = re.compile(b".*".join(re.escape(x) for x in pattern.encode().split(b"%")), re.DOTALL | (re.IGNORECASE if nocase else 0))
    return rx.fullmatch(v) is not None


def rows_of(env, predicate):
    return [k for k, doc in enumerate(env.docs) if predicate(doc)]


def where_rows(env, specs, **kw):
    """The documents' numbers ``Window.where`` keeps over the whole stream"""
    got, seen = [], 0
    for win in env.stream():
        sel = win.where(specs, **kw)
        got += [seen + r for r in sel.rows.cpu().tolist()]
        seen += win.n_documents
    assert seen == len(env.docs)
    return got


@gpu
def test_where_contains_suffix_like(env):
    m = lambda doc: text(doc)
    assert where_rows(env, [("/message", "contains", "timeout")]) == rows_of(env, lambda d: m(d) is not None and b"timeout" in m(d))
    assert 10 in where_rows(env, [("/message", "contains", "timeout é")]) and 30 not in where_rows(env, [("/message", "contains", "timeout")])
    assert where_rows(env, [("/message", "contains", 'a"b')]) == rows_of(env, lambda d: m(d) is not None and b'a"b' in m(d))
    assert 20 in where_rows(env, [("/message", "contains", b"\ttab")])
    assert where_rows(env, [("/message", "icontains", "TIMEout")]) == rows_of(env, lambda d: m(d) is not None and b"timeout" in m(d).lower())
    assert where_rows(env, [("/message", "suffix", ".png")]) == rows_of(env, lambda d: m(d) is not None and m(d).endswith(b".png"))
    assert where_rows(env, [("/message", "isuffix", ".PnG")]) == rows_of(env, lambda d: m(d) is not None and m(d).lower().endswith(b".png"))
    for pattern in ("GET %.png", "%time%out%", "timeout", "%o%", "GET %img%a%", "100%", "%é%"):
        assert where_rows(env, [("/message", "like", pattern)]) == rows_of(env, lambda d: m(d) is not None and like(pattern, m(d))), pattern
        assert where_rows(env, [("/message", "ilike", pattern.upper())]) == \
            rows_of(env, lambda d: m(d) is not None and like(pattern.upper(), m(d), True)), pattern
    with pytest.raises(ValueError):
        where_rows(env, [("/message", "like", "a_b")])
    with pytest.raises(ValueError):
        where_rows(env, [("/message", "like", "a%%b")])


@gpu
def test_where_not_any_and_mixed(env):
    m = lambda doc: text(doc)
    has = lambda d, x: m(d) is not None and x in m(d)
    # ("not", ...) also passes a document without the string: a number, a missing key, a verdict code
    got = where_rows(env, [("not", ("/message", "contains", "timeout"))])
    assert got == rows_of(env, lambda d: not has(d, b"timeout")) and 30 in got
    assert where_rows(env, [("/message", "contains", "timeout"), ("/message", "suffix", ".png")], any=True) == \
        rows_of(env, lambda d: has(d, b"timeout") or (m(d) is not None and m(d).endswith(b".png")))
    # several patterns on one column, another column, numeric and cast predicates next to them
    lat = lambda d: d is not None and d.get("latency", -1)
    assert where_rows(env, [("/message", "contains", "time"), ("not", ("/message", "icontains", "OUT:")), ("/status", "like", "%r%"),
                            ("/latency", ">", 100)]) == \
        rows_of(env, lambda d: has(d, b"time") and b"out:" not in m(d).lower() and b"r" in text(d, "status") and lat(d) > 100)
    assert where_rows(env, [("/message", "contains", "o"), ("/price", ">=", 40.5), ("/latency", "<", 400)], cast={"/price": "number"}) == \
        rows_of(env, lambda d: has(d, b"o") and float(d["price"]) >= 40.5 and lat(d) < 400)
    assert where_rows(env, [("/price", "suffix", "1.5"), ("/price", "<", 50)], cast={"/price": "number"}) == \
        rows_of(env, lambda d: d is not None and d["price"].endswith("1.5") and float(d["price"]) < 50)
    # an existing spec list gives the same rows as before
    assert where_rows(env, [("/status", "==", "error"), ("/latency", ">", 250)]) == \
        rows_of(env, lambda d: d is not None and d["status"] == "error" and d["latency"] > 250)
    assert where_rows(env, [("/message", "prefix", "time")]) == rows_of(env, lambda d: m(d) is not None and m(d).startswith(b"time"))
    with pytest.raises(ValueError):  # 18 columns of match records
        where_rows(env, [(name, "contains", "x%d" % j) for j in range(9) for name in ("/message", "/status")])


@gpu
def test_match_records_and_grep(env):
    import torch

    seen = 0
    for win in env.stream():
        D = win.n_documents
        docs, lines = env.docs[seen:seen + D], env.lines[seen:seen + D]
        specs = [b"timeout", ([b"GET ", b".png"], {"at_start", "at_end", "nocase"})]
        tspecs = [b"timeout", ([b"GET ", b".png"], tmm.AT_START | tmm.AT_END | tmm.NOCASE)]
        fields, d_select = win.match("/message", specs)
        assert tuple(fields.shape) == (2, D, 2) and fields.dtype == torch.int64 and fields.is_cuda and tuple(d_select.shape) == (48,)
        rec = np.ascontiguousarray(fields.cpu().numpy()).view(tmm.FIELD).reshape(2, D)
        sel = tmm.SelectResult.from_buffer_copy(d_select.cpu().numpy().tobytes())
        n_found = 0
        for p, s in enumerate(tspecs):
            for k, doc in enumerate(docs):
                at = None if text(doc) is None else tmm.py_match(text(doc), s)
                want = (0, 0xFFFFFFFF, 0, 0, 20) if at is None else (at, 0xFFFFFFFF, ord("l"), 0, 0)
                assert tuple(rec[p, k].tolist()) == want, (p, seen + k)
                n_found += at is not None
        assert (sel.code, sel.n_documents, sel.n_paths, sel.n_found) == (0, D, 2, n_found)
        # grep over the window's lines: the text as it is written, escapes and all
        grep, _ = win.match("", [b"timeout", b"\\u0074imeout", ([b'"status"', b"error"], set())], raw=True)
        grec = np.ascontiguousarray(grep.cpu().numpy()).view(tmm.FIELD).reshape(3, D)
        for p, s in enumerate((b"timeout", b"\\u0074imeout", ([b'"status"', b"error"], 0))):
            for k, (doc, line) in enumerate(zip(docs, lines)):
                at = None if doc is None else tmm.py_match(line, s)
                assert (grec[p, k]["code"] == 0) == (at is not None) and (at is None or grec[p, k]["bits"] == at), (p, seen + k)
        # on the chosen rows of a selection: the same records, taken
        chosen = win.where([("/status", "==", "error")])
        again, _ = chosen.match("/message", specs)
        assert again.equal(fields[:, chosen.rows.long()])
        seen += D
    assert seen == len(env.docs)


@gpu
def test_list_column_and_element_fields(env):
    seen = 0
    is_str = lambda v: isinstance(v, str)
    for win in env.stream():
        D = win.n_documents
        docs = env.docs[seen:seen + D]
        tags = win.elements("/tags").where([(0, "contains", "time")]).to_python()
        want = [None if d is None or not isinstance(d["tags"], list) else [t for t in d["tags"] if is_str(t) and "time" in t] for d in docs]
        assert tags == want
        tags = win.elements("/tags").where([("not", (0, "ilike", "%PNG"))]).to_python()
        want = [None if d is None or not isinstance(d["tags"], list) else [t for t in d["tags"] if not (is_str(t) and t.lower().endswith("png"))]
                for d in docs]
        assert tags == want
        items = win.elements("/items").select(["/name", "/qty"]).where([("/name", "suffix", "png"), ("/qty", ">=", 1)]).to_python()
        want = [None if d is None else [{"/" + k: v for k, v in it.items()} for it in d["items"]
                                        if is_str(it.get("name")) and it["name"].endswith("png") and isinstance(it.get("qty"), int) and it["qty"] >= 1] for d in docs]
        assert items == want
        seen += D
    assert seen == len(env.docs)
