"""``bucket``, ``group_by``, ``stats(by=[...])``, ``GroupKeys.order()`` and ``RunningGroups`` of the record views
(mojo_simdjson_amd/document_stream.py) against json.loads, datetime and a plain Python group-by.

The corpus is 2 000 log lines: /ts with mixed UTC offsets and fraction widths (none, 1, 3, 6 and 9 digits) and, every 19th
line, a timestamp before 1970, where the floor of a bucket differs from truncation; /code written as 200, 200.0 and 2e2 (one
group) next to other numbers; /status missing in every 11th line; /latency_ms an integer, missing in every 7th line.  The model
parses every line with json.loads, the timestamps with a regular expression and datetime, and groups with a dict.
"""
import datetime
import json
import random
import re
from fractions import Fraction

import pytest

from tests import test_validate_documents as tvd

pytestmark = pytest.mark.gpu

LINES = 2000
POINTERS = ["/ts", "/code", "/status", "/latency_ms"]
MINUTE = datetime.timedelta(minutes=1)
CAST = {"/ts": ("timestamp", "ms")}
EPOCH = datetime.datetime(1970, 1, 1, tzinfo=datetime.timezone.utc)
_TS = re.compile(r"(\d{4})-(\d\d)-(\d\d)T(\d\d):(\d\d):(\d\d)(?:\.(\d+))?(Z|[+-]\d\d:\d\d)$")


def corpus():
    rng = random.Random(2024)
    lines = []
    for k in range(LINES):
        h, m, s = rng.randrange(10, 14), rng.randrange(0, 4), rng.randrange(60)
        frac = ["", ".5", ".123", ".000999", ".999999999"][k % 5]
        if k % 19 == 0:
            ts = "1969-12-31T23:%02d:%02d%sZ" % (56 + m, s, frac)
        else:
            off_h, off_m = rng.choice([(0, 0), (2, 0), (-4, -30), (5, 45)])
            zone = "Z" if (off_h, off_m) == (0, 0) and k % 2 else "%s%02d:%02d" % ("-" if off_h < 0 else "+", abs(off_h), abs(off_m))
            ts = "2024-05-01T%02d:%02d:%02d%s%s" % (h, m, s, frac, zone)
        code = rng.choice(["200", "200.0", "2e2", "404", "500", "503.5", "-1"])
        doc = ['"ts":"%s"' % ts, '"code":%s' % code]
        if k % 11:
            doc.append('"status":"%s"' % rng.choice(["ok", "error", "warn", "d\\u00e9bil"]))
        if k % 7:
            doc.append('"latency_ms":%d' % rng.randrange(-50, 100000))
        lines.append("{" + ",".join(doc) + "}")
    return lines


def millis(ts):
    """An RFC 3339 timestamp as milliseconds since 1970, the fraction cut to three digits"""
    Y, M, D, h, m, s, frac, zone = _TS.match(ts).groups()
    whole = datetime.datetime(int(Y), int(M), int(D), int(h), int(m), int(s), tzinfo=datetime.timezone.utc) - EPOCH
    seconds = whole.days * 86400 + whole.seconds
    if zone != "Z":
        seconds -= (1 if zone[0] == "+" else -1) * (int(zone[1:3]) * 3600 + int(zone[4:6]) * 60)
    return seconds * 1000 + int(((frac or "") + "000")[:3])


def canonical(v):
    f = Fraction(v)
    return int(f) if f.denominator == 1 else float(v)


class Model:
    def __init__(self, lines):
        self.docs = [json.loads(line) for line in lines]

    def part(self, doc, key, origin=0):
        if isinstance(key, str):
            return doc.get(key[1:])
        path, kind = key[0], key[1]
        v = doc.get(path[1:])
        if kind == "number":
            return None if v is None else canonical(v)
        ms = millis(v)
        return origin + (ms - origin) // 60000 * 60000

    def groups(self, keys, nulls=False, origin=0):
        """-> (the key tuples in the order of first appearance, the code per line: -1 without a key)"""
        seen, codes = {}, []
        for doc in self.docs:
            key = tuple(self.part(doc, k, origin) for k in keys)
            if None in key and not nulls:
                codes.append(-1)
            else:
                codes.append(seen.setdefault(key, len(seen)))
        return list(seen), codes

    def stats(self, keys):
        values, codes = self.groups(keys)
        out = [{"key": v, "/latency_ms": {"n_rows": 0, "n_values": 0, "sum": None, "min": None, "max": None, "flags": 0}} for v in values]
        for doc, c in zip(self.docs, codes):
            if c < 0:
                continue
            r = out[c]["/latency_ms"]
            r["n_rows"] += 1
            v = doc.get("latency_ms")
            if v is not None:
                r["n_values"] += 1
                r["sum"], r["min"], r["max"] = (r["sum"] or 0) + v, v if r["min"] is None else min(r["min"], v), v if r["max"] is None else max(r["max"], v)
        return out


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
def lines():
    return corpus()


def windows(dev, lines, window):
    from mojo_simdjson_amd.document_stream import DocumentStream

    data = ("\n".join(lines) + "\n").encode()
    return DocumentStream(dev, tvd.upload(dev, data), len(data), window=window, select=POINTERS)


def test_the_corpus_on_the_host(lines):
    m = Model(lines)
    assert millis("1969-12-31T23:59:59.999Z") == -1 and millis("1970-01-01T02:00:00.5+02:00") == 500
    minutes = {m.part(d, ("/ts", "bucket")) for d in m.docs}
    assert min(minutes) < 0 and any(millis(d["ts"]) < 0 and millis(d["ts"]) % 60000 for d in m.docs)
    assert {canonical(d["code"]) for d in m.docs} == {200, 404, 500, 503.5, -1}
    assert sum("status" not in d for d in m.docs) > 100


def test_bucket_and_group_by_one_window(dev, lines):
    import torch

    from mojo_simdjson_amd.document_stream import number_column

    (win,) = list(windows(dev, lines, 1 << 22))
    m = Model(lines)
    # bucket: every line's minute, by a timedelta and by its milliseconds; an origin as a datetime and as an int
    want = [m.part(d, ("/ts", "bucket")) for d in m.docs]
    for width in (MINUTE, 60000):
        records, d_select = win.bucket("/ts", width, cast=("timestamp", "ms"))
        values, valid = number_column(records, torch.int64)
        assert bool(valid.all()) and values.cpu().tolist() == want
    origin = datetime.datetime(2024, 5, 1, 0, 0, 30, tzinfo=datetime.timezone.utc)
    shifted = [m.part(d, ("/ts", "bucket"), millis("2024-05-01T00:00:30Z")) for d in m.docs]
    values, _ = number_column(win.bucket("/ts", MINUTE, origin, cast=("timestamp", "ms"))[0], torch.int64)
    assert values.cpu().tolist() == shifted and shifted != want
    values, valid = number_column(win.bucket("/code", 100)[0], torch.int64)
    assert values.cpu().tolist() == [int(Fraction(d["code"]) // 100 * 100) for d in m.docs] and bool(valid.all())
    with pytest.raises(ValueError):
        win.bucket("/code", MINUTE)
    with pytest.raises(ValueError):
        win.bucket("/ts", datetime.timedelta(microseconds=1500), cast=("timestamp", "ms"))

    # group_by: one string key is categories; a number key merges 200, 200.0 and 2e2; three keys at once
    cats, g = win.categories("/status"), win.group_by(["/status"])
    assert g.codes.cpu().tolist() == cats.codes.cpu().tolist() and g.values() == [(v,) for v in cats.values()] and g.key_width == 5
    assert g.first.cpu().tolist() == cats.first.cpu().tolist() and g.counts().cpu().tolist() == cats.counts().cpu().tolist()
    g = win.group_by([("/code", "number")])
    values, codes = m.groups([("/code", "number")])
    assert g.values() == values and g.codes.cpu().tolist() == codes and [type(v[0]) for v in g.values()] == [type(v[0]) for v in values]
    keys = ["/status", ("/code", "number"), ("/ts", "bucket", MINUTE)]
    g = win.group_by(keys, cast=CAST)
    values, codes = m.groups(keys)
    assert g.values() == values and g.codes.cpu().tolist() == codes and g.n_distinct == len(values) and g.key_width == 27
    assert g.counts().cpu().tolist() == [codes.count(c) for c in range(len(values))]
    # no value as a group of its own
    g = win.group_by([("/status", "string", {"nulls"}), ("/code", "number")])
    values, codes = m.groups(["/status", ("/code", "number")], nulls=True)
    assert g.values() == values and g.codes.cpu().tolist() == codes and min(codes) == 0 and any(v[0] is None for v in values)

    # the groups in key order, the first key major
    g = win.group_by([("/code", "number"), ("/ts", "bucket", 60000)], cast=CAST)
    values = g.values()
    in_order = [values[c] for c in g.order().sorted.cpu().tolist()]
    assert in_order == sorted(values, key=lambda v: (Fraction(v[0]), v[1])) and len(in_order) == len(m.groups([("/code", "number"), ("/ts", "bucket")])[0])


def test_stats_by_a_list(dev, lines):
    import torch

    (win,) = list(windows(dev, lines, 1 << 22))
    m = Model(lines)
    one, listed = win.stats(["/latency_ms"], by="/status"), win.stats(["/latency_ms"], by=["/status"])
    assert one.n_groups == listed.n_groups and torch.equal(one.records, listed.records) and one.n_ungrouped == listed.n_ungrouped
    assert [r["key"] for r in listed.to_python()] == [(r["key"],) for r in one.to_python()]
    keys = ["/status", ("/ts", "bucket", MINUTE)]
    got = win.stats(["/latency_ms"], by=keys, cast=CAST)
    want = m.stats(keys)
    assert got.to_python() == want
    assert got.n_ungrouped == sum("status" not in d for d in m.docs) and got.keys.n_distinct == len(want)
    sel = win.where([("/code", "==", 200)])
    kept = Model([line for line, d in zip(lines, m.docs) if d["code"] == 200])
    assert sel.stats(["/latency_ms"], by=keys, cast=CAST).to_python() == kept.stats(keys)


def test_running_groups_over_three_windows(dev, lines):
    from mojo_simdjson_amd.document_stream import RunningGroups

    data_len = sum(len(line) + 1 for line in lines)
    keys = ["/status", ("/code", "number"), ("/ts", "bucket", MINUTE)]
    rg = RunningGroups(dev, keys, dict_capacity=4)
    merged, seen, n_windows, codes = {}, 0, 0, []
    for win in windows(dev, lines, (data_len // 3 + 4096) // 16 * 16):
        stats = win.stats(["/latency_ms"], by=keys, cast=CAST, dictionary=rg)
        assert stats.n_groups == rg.n_distinct
        codes += stats.keys.codes.cpu().tolist()
        for g, r in enumerate(stats.to_python()):
            r = r["/latency_ms"]
            a = merged.setdefault(g, {"n_rows": 0, "n_values": 0, "sum": None, "min": None, "max": None, "flags": 0})
            a["n_rows"] += r["n_rows"]
            a["n_values"] += r["n_values"]
            if r["n_values"]:   # (merging two windows' records: counts add, 'l' sums add, min and max merge)
                a["sum"] = (a["sum"] or 0) + r["sum"]
                a["min"] = r["min"] if a["min"] is None else min(a["min"], r["min"])
                a["max"] = r["max"] if a["max"] is None else max(a["max"], r["max"])
        frozen = win.group_by(keys, cast=CAST, dictionary=rg, frozen=True)
        assert frozen.codes.cpu().tolist() == stats.keys.codes.cpu().tolist() and rg.n_distinct == stats.n_groups
        seen += win.n_documents
        n_windows += 1
    assert seen == len(lines) and n_windows >= 3
    m = Model(lines)
    want = m.stats(keys)
    values, want_codes = m.groups(keys)
    assert rg.values() == values and codes == want_codes
    assert [merged[g] for g in range(len(want))] == [w["/latency_ms"] for w in want]
    in_order = [values[c] for c in rg.order().sorted.cpu().tolist()]
    status_code = {v: c for c, v in enumerate(rg.strings[0].values())}
    assert in_order == sorted(values, key=lambda v: (status_code[v[0]], Fraction(v[1]), v[2]))
