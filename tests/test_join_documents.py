"""``Window.join`` / ``RowSelection.join`` end to end (mojo_simdjson_amd/document_stream.py): two NDJSON streams on the device
-- events with ``/user``, users with ``/id`` -- joined through ``strings`` or ``raw``, a ``RunningDictionary`` and
msj_join_rows_device, and the joined rows taken on both sides.  The yardstick is ``json.loads`` over both files and a double
loop in Python; the values of both sides of EVERY pair are compared, the missing right side of how="left" included."""
import json

import pytest

pytestmark = pytest.mark.gpu

HOWS = ("inner", "left", "semi", "anti")


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


def raw_key(v):
    """compact JSON text, as json.dumps writes the values used here"""
    return json.dumps(v, ensure_ascii=False, separators=(",", ":"))


def py_join(left, right, lkey, rkey, how, key_of):
    """-> [(left doc, right doc or None)] of the definition; key_of(doc, name): the key, or None for a row without one"""
    out = []
    for l in left:
        k = key_of(l, lkey)
        match = [r for r in right if k is not None and key_of(r, rkey) == k]
        if how == "inner":
            out += [(l, r) for r in match]
        elif how == "left":
            out += [(l, r) for r in match] or [(l, None)]
        elif how == "semi":
            out += [(l, None)] if match else []
        else:
            out += [] if match else [(l, None)]
    return out


def string_key(doc, name):
    return doc[name] if isinstance(doc.get(name), str) else None


def raw_text_key(doc, name):
    return raw_key(doc[name]) if name in doc else None


def flat(pairs, lnames, rnames, with_right):
    return [(tuple(l.get(n) for n in lnames), tuple((r or {}).get(n) for n in rnames) if with_right else None) for l, r in pairs]


def events_and_users():
    events = [{"user": "u%d" % (k * 7 % 23), "n": k} for k in range(300)]
    events[5] = {"n": 5}                       # no key
    events[9] = {"user": 9, "n": 9}            # not a string: no key by="string"
    events[12] = {"user": "nobody", "n": 12}   # a value the users do not hold
    events[13] = {"user": "ü ber", "n": 13}
    users = [{"id": "u%d" % k, "name": "name %d" % k} for k in range(0, 20)]
    users += [{"id": "u3", "name": "the second u3"}, {"id": 9, "name": "nine"}, {"name": "no id"}, {"id": "unused", "name": "x"},
              {"id": "ü ber", "name": "umlaut"}]
    return events, users


@pytest.mark.parametrize("how", HOWS)
def test_join_on_strings(dev, how):
    import torch

    from mojo_simdjson_amd.document_stream import JoinedRows, RowSelection

    events, users = events_and_users()
    ewin = next(windows_of(dev, events, ["/user", "/n"]))
    uwin = next(windows_of(dev, users, ["/id", "/name"]))
    joined = ewin.join(uwin, "/user", "/id", how=how)
    want = py_join(events, users, "user", "id", how, string_key)
    with_right = how in ("inner", "left")
    assert isinstance(joined, JoinedRows) and isinstance(joined.left, RowSelection) and joined.n_pairs == len(want) == joined.result.n_pairs
    assert (joined.right is not None) == with_right and joined.left_rows.is_cuda and joined.left_rows.dtype == torch.int32
    assert joined.to_python(["/user", "/n"], ["/id", "/name"]) == flat(want, ("user", "n"), ("id", "name"), with_right)
    assert [events[l] for l in joined.left.rows.cpu().tolist()] == [l for l, _ in want]
    if with_right:
        assert [users[r] if r >= 0 else None for r in joined.right.rows.cpu().tolist()] == [r for _, r in want]
        assert joined.right.strings("/name")[2].cpu().tolist() == [r is not None for _, r in want]
    off = joined.offsets.cpu().tolist()
    assert off[0] == 0 and off[-1] == len(want) and len(off) == len(events) + 1
    assert [b - a for a, b in zip(off, off[1:])] == [sum(1 for l, _ in want if l is e) for e in events]


@pytest.mark.parametrize("how", HOWS)
def test_join_on_raw_text(dev, how):
    """Integer ids, by="raw": equal compact JSON text is the key -- 7 matches 7, neither 7.0 nor "7"; a container is a key too"""
    events = [{"user": k % 11, "n": k} for k in range(120)]
    events[3] = {"user": 7.0, "n": 3}
    events[4] = {"user": "7", "n": 4}
    events[6] = {"n": 6}
    events[8] = {"user": [1, {"a": 2}], "n": 8}
    users = [{"id": k, "name": "name %d" % k} for k in range(9)] + [{"id": "7", "name": "the string"}, {"id": [1, {"a": 2}], "name": "a list"},
                                                                    {"id": 7, "name": "seven again"}]
    ewin = next(windows_of(dev, events, ["/user", "/n"]))
    uwin = next(windows_of(dev, users, ["/id", "/name"]))
    # (the files are written with blanks behind ':' and ',': compact=True takes them out of the container's text)
    joined = ewin.join(uwin, "/user", "/id", how=how, by="raw")
    want = py_join(events, users, "user", "id", how, raw_text_key)
    assert joined.to_python(["/n"], ["/name"]) == flat(want, ("n",), ("name",), how in ("inner", "left"))
    with pytest.raises(ValueError):
        ewin.join(uwin, "/user", "/id", by="number")


def test_self_join_and_selections(dev):
    events, users = events_and_users()
    ewin = next(windows_of(dev, events, ["/user", "/n"]))
    uwin = next(windows_of(dev, users, ["/id", "/name"]))
    few = events[:40]
    joined = ewin.take(ewin.where([("/n", "<", 40)]).rows).join(ewin.where([("/n", "<", 40)]), "/user")
    want = py_join(few, few, "user", "user", "inner", string_key)
    assert joined.to_python(["/n"], ["/n"]) == flat(want, ("n",), ("n",), True) and len(want) > len(few)
    whole = ewin.join(ewin, "/user", how="semi")
    assert whole.n_pairs == sum(1 for e in events if isinstance(e.get("user"), str))
    # selections of both sides: the rows are the windows' document numbers
    late, named = ewin.where([("/n", ">=", 250)]), uwin.where([("/name", "prefix", "name 1")])
    joined = late.join(named, "/user", "/id", how="left")
    lwant = [e for e in events if e["n"] >= 250]
    rwant = [u for u in users if u["name"].startswith("name 1")]
    want = py_join(lwant, rwant, "user", "id", "left", string_key)
    assert joined.to_python(["/n"], ["/name"]) == flat(want, ("n",), ("name",), True)
    assert joined.left.rows.cpu().tolist() == [events.index(l) for l, _ in want]
    assert joined.right.rows.cpu().tolist() == [users.index(r) if r is not None else -1 for _, r in want]


def test_shared_dictionary_across_windows_and_the_capacity_retry(dev):
    from mojo_simdjson_amd.document_stream import RunningDictionary

    events, users = events_and_users()
    uwin = next(windows_of(dev, users, ["/id", "/name"]))
    rd = RunningDictionary(dev, dict_capacity=4, bytes_capacity=16)
    seen, windows, sizes = 0, 0, []
    for ewin in windows_of(dev, events, ["/user", "/n"], window=4096):
        mine = events[seen:seen + ewin.n_documents]
        joined = ewin.join(uwin, "/user", "/id", how="left", dictionary=rd, pairs_capacity=1)   # clipped: repeated once
        want = py_join(mine, users, "user", "id", "left", string_key)
        assert joined.to_python(["/user", "/n"], ["/name"]) == flat(want, ("user", "n"), ("name",), True), windows
        assert joined.result.code == 0 and joined.n_pairs == len(want) > 1
        seen += ewin.n_documents
        windows += 1
        sizes.append(rd.n_distinct)
    assert windows >= 2 and seen == len(events)
    # one dictionary: the users' ids first, then the values only the events hold; nothing is numbered twice
    values = rd.values()
    assert len(set(values)) == len(values) == sizes[-1] and "nobody" in values and "unused" in values and sizes == sorted(sizes)
    assert values[:len({u["id"] for u in users if isinstance(u.get("id"), str)})] == list(dict.fromkeys(u["id"] for u in users if isinstance(u.get("id"), str)))
