"""A byte column as codes plus distinct values on the device (msj_dictionary_device, csrc/dictionary_kernel.hip).

Expected values come from the host twin of the same arithmetic (tests/dictionary_math_host.cpp), which
tests/test_dictionary_math.py holds against a yardstick written in Python.  Device output is compared with the twin over the
WHOLE d_codes, d_dict_offsets, d_dict_first and d_dict_bytes arrays (both start from the same fill, with 64 bytes of canary
behind each capacity, so a store the twin does not make shows) and over the result -- but for max_probe, which depends on
which row reached a slot first and is held against its bounds.  Columns are generated and uploaded; the end-to-end tests
run the real chain through DocumentStream.

The kernels' constants (csrc/dictionary_kernel.hip) are named below as the shapes use them.
"""
import json

import numpy as np
import pytest

from tests import test_dictionary_math as tdc
from tests import test_tape_documents as ttd
from tests import test_validate_documents as tvd

pytestmark = pytest.mark.gpu

B = 256                  # kRows: rows per workgroup of the kernels over the rows
ROW_GRID = 4096 * B      # kGridBlocks = 4096 blocks of kRows rows, `v += gridDim.x`
SCAN_CHUNK = 1024        # wave_ops.h, scan_in_place: blocks of rows per chunk of the running sums
LONG_ROW = 512           # kLongRow: a row of MORE bytes than this is hashed and compared by a wave, not by its lane
LONG_CAP = 1024          # kLongCap: entries of the list of long rows; a long row past it is carried by its own wave
PIECE = 16384            # kPiece: bytes of aligned output a workgroup of dc_copy takes at a time
MSJ_CAPACITY, BAD_ARGUMENT = 1, -1
WEAK = tdc.WEAK


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
def dtwin():
    return tdc.load_twin()


class OnDevice:
    """A tdc.Column uploaded, padded so that no tensor is empty"""

    def __init__(self, dev, col):
        self.rows, self.bytes_len = col.rows, int(col.data.size)
        self.d_offsets = ttd.to_device(dev, col.offsets)
        self.d_valid = ttd.to_device(dev, np.concatenate([col.valid, np.zeros(8, dtype=np.uint8)]))
        self.d_bytes = ttd.to_device(dev, np.concatenate([col.data, np.zeros(16, dtype=np.uint8)]))


def device_dictionary(dev, a, want, n_rows=None, shift=0):
    """msj_dictionary_device with the twin's capacities and flags, its arrays filled like the twin's with their canaries;
    n_rows: the row count as a word on the device; shift: d_dict_bytes starts that many bytes off a 16-byte boundary
    -> tdc.Encoded"""
    import torch

    layout_only = want.dict_offsets is None
    codes, d_off, d_first, d_bytes = tdc.filled(want.rows, want.dict_capacity, want.dict_bytes_capacity, layout_only)
    up = lambda x: torch.from_numpy(x).to(dev.device)
    t_codes = up(codes)
    t_off = t_first = t_all = t_bytes = None
    if not layout_only:
        t_off, t_first = up(d_off.view(np.int64)), up(d_first.view(np.int32))
        t_all = up(np.concatenate([np.full(shift, tdc.FILL, dtype=np.uint8), d_bytes]))
        t_bytes = t_all[shift:]
    d_n_rows = up(np.array([n_rows], dtype=np.uint64).view(np.int64)) if n_rows is not None else None
    res, *_ = dev.dictionary(a.d_offsets, a.d_bytes, a.d_valid, rows=want.rows, d_n_rows=d_n_rows, bytes_len=a.bytes_len, d_codes=t_codes,
                             d_dict_offsets=t_off, d_dict_first=t_first, d_dict_bytes=t_bytes, dict_capacity=want.dict_capacity,
                             dict_bytes_capacity=want.dict_bytes_capacity, values=not layout_only, weak_hash=bool(want.res.flags & WEAK))
    if layout_only:
        return tdc.Encoded(res, t_codes.cpu().numpy(), None, None, None, want.rows, 0, 0)
    assert bool((t_all[:shift] == tdc.FILL).all())
    return tdc.Encoded(res, t_codes.cpu().numpy(), t_off.cpu().numpy().view(np.uint64), t_first.cpu().numpy().view(np.uint32),
                       t_bytes.cpu().numpy(), want.rows, want.dict_capacity, want.dict_bytes_capacity)


def same(got, want, where=None):
    """The device's result and every array are the twin's, fill and canary included"""
    assert got.summary() == want.summary(), (where, got.summary(), want.summary())
    longest, R = int(got.res.max_probe), int(want.res.n_rows)
    assert (longest == 0) == (want.res.max_probe == 0) and longest <= max(tdc.MIN_SLOTS, 4 * R), (where, longest)
    for name in ("codes", "dict_offsets", "dict_first", "dict_bytes"):
        x, y = getattr(got, name), getattr(want, name)
        if y is None:
            assert x is None
            continue
        bad = np.nonzero(x != y)[0]
        assert bad.size == 0, (where, name, int(bad[0]), x[bad[:4]].tolist(), y[bad[:4]].tolist(), bad.size)


def check(dev, dtwin, col, flags=(0,), layouts=(True, False), shift=0, where=None, a=None, **kw):
    """The device against the twin, layout-only and with the dictionary -> (the last twin Encoded, the last device one)"""
    a = OnDevice(dev, col) if a is None else a
    for f in flags:
        for layout_only in layouts:
            want = tdc.twin_dictionary(dtwin, col, flags=f, layout_only=layout_only, **kw)
            got = device_dictionary(dev, a, want, n_rows=kw.get("n_rows"), shift=shift)
            same(got, want, (where, f, layout_only))
    return want, got


def numbered(n, width=7, start=0):
    """n distinct values of `width` decimal digits, generated: -> tdc.Column"""
    k = np.arange(start, start + n, dtype=np.int64)
    digits = (k[:, None] // 10 ** np.arange(width - 1, -1, -1, dtype=np.int64)[None, :]) % 10 + 48
    return tdc.Column(np.arange(n + 1, dtype=np.uint64) * width, np.ones(n, dtype=np.uint8), digits.astype(np.uint8).tobytes())


@pytest.mark.parametrize("n", [0, 1, B - 1, B, B + 1])
def test_row_counts(dev, dtwin, n):
    """No row, one row, and the block border: values that repeat with a period that is no divisor of the block, a null row
    and an empty value among them; both hashes."""
    values = [None if k % 11 == 5 else b"" if k % 7 == 3 else b"value-%d" % (k % 37) for k in range(n)]
    want, _ = check(dev, dtwin, tdc.column_of(values), flags=(0, WEAK), where=n)
    tdc.check(want, values, int(want.res.flags))


def test_chains_that_wrap(dev, dtwin):
    """300 values of lengths 0 .. 7 under MSJ_DICTIONARY_WEAK_HASH: four chains of about 75 that start in the table's last
    four slots and wrap through slot 0, every slot decided by the byte compare; then 300 rows of 3 values the same way."""
    values = tdc.weak_values()
    want, got = check(dev, dtwin, tdc.column_of(values + values[::-3]), flags=(WEAK, 0), shift=5)
    assert want.res.n_distinct == 300
    _, weak = check(dev, dtwin, tdc.column_of(values), flags=(WEAK,))
    assert weak.res.max_probe >= 75   # (the longest chain holds 75 values or more, and its last value walked all of it)
    check(dev, dtwin, tdc.column_of([(b"red", b"green", b"blue")[k % 3] for k in range(300)]), flags=(WEAK, 0))


@pytest.mark.parametrize("n_values", [3, 1])
def test_hot_column_is_reproducible(dev, dtwin, n_values):
    """70 000 rows over 3 values interleaved, and over 1: thousands of lanes meet in the same slot.  Run twice: the two
    outputs are bit-identical and the twin's."""
    names = (b"active", b"suspended", b"closed")[:n_values]
    col = tdc.column_of([names[k % n_values] for k in range(70000)])
    a = OnDevice(dev, col)
    want = tdc.twin_dictionary(dtwin, col)
    runs = [device_dictionary(dev, a, want) for _ in range(2)]
    for got in runs:
        same(got, want, n_values)
    for name in ("codes", "dict_offsets", "dict_first", "dict_bytes"):
        assert getattr(runs[0], name).tobytes() == getattr(runs[1], name).tobytes(), name
    assert want.res.n_distinct == n_values and want.dict_first[:n_values].tolist() == list(range(n_values))


@pytest.mark.parametrize("n", [SCAN_CHUNK * B + 1, ROW_GRID + 1 + 300])
def test_all_distinct_past_the_scan_chunk_and_the_row_grid(dev, dtwin, n):
    """All-distinct short values, generated: 262 145 rows reach the second chunk of the block-sum scan, 1 048 577 + 300
    the second trip of the row grid.  Every row is its own first row."""
    col = numbered(n)
    want, _ = check(dev, dtwin, col, layouts=(False,), where=n)
    assert want.res.n_distinct == n and want.res.dict_bytes == 7 * n
    assert np.array_equal(want.codes[:n], np.arange(n, dtype=np.int32)) and want.dict_bytes[:7 * n].tobytes() == col.data.tobytes()


def test_rows_around_the_long_threshold(dev, dtwin):
    """Lengths kLongRow - 1 .. + 2, each twice equal and once with another last byte, short rows and null rows between
    them: a value hashed by a lane over LDS and one hashed by a wave agree where they must."""
    values = []
    for n in (LONG_ROW - 1, LONG_ROW, LONG_ROW + 1, LONG_ROW + 2):
        base = bytes((3 * j + n) & 0xFF for j in range(n))
        values += [base, b"short", base[:-1] + b"\xff", None, base, b""]
    want, _ = check(dev, dtwin, tdc.column_of(values), flags=(0, WEAK), shift=3)
    assert want.res.n_distinct == 2 * 4 + 2
    tdc.check(want, values, int(want.res.flags))


def test_one_mebibyte_values(dev, dtwin):
    """Two equal values of 1 MiB and a third that differs in its last byte: two codes; the dictionary's two long entries
    are copied in pieces of kPiece by the grid."""
    rng = np.random.default_rng(11)
    big = rng.integers(0, 256, 1 << 20, dtype=np.uint8).tobytes()
    values = [big, b"x", big[:-1] + bytes([big[-1] ^ 1]), big]
    want, _ = check(dev, dtwin, tdc.column_of(values), layouts=(False,), shift=9)
    assert want.codes[:4].tolist() == [0, 1, 2, 0] and want.res.dict_bytes == 2 * (1 << 20) + 1 > 100 * PIECE


def test_long_values_that_differ_in_one_byte(dev, dtwin):
    """Equal-length long values that differ from the first in exactly one byte: at every offset 0 .. 130 and at 64 Ki + r
    for r = 0 .. 63 behind a few thousand -- every lane of a 64-lane step and both ends of the 8-byte words.  All come
    out distinct, and a copy of each equals its original.  Under the weak hash every pair is decided by the wave compare."""
    n = (64 << 10) + 64 + 3000
    rng = np.random.default_rng(12)
    base = rng.integers(0, 256, n, dtype=np.uint8)
    at = list(range(131)) + [(64 << 10) + r for r in range(64)]
    rows = np.tile(base, (1 + len(at), 1))
    for j, p in enumerate(at):
        rows[1 + j, p] ^= 0x10
    rows = np.concatenate([rows, rows[::-1]])
    R = rows.shape[0]
    col = tdc.Column(np.arange(R + 1, dtype=np.uint64) * n, np.ones(R, dtype=np.uint8), rows.tobytes())
    want, _ = check(dev, dtwin, col, layouts=(False,))
    half = R // 2
    assert want.res.n_distinct == half and want.codes[:R].tolist() == list(range(half)) + list(range(half))[::-1]
    few = tdc.Column(col.offsets[:41], col.valid[:40], rows[:40].tobytes())
    check(dev, dtwin, few, flags=(WEAK,), layouts=(False,))


@pytest.mark.parametrize("extra", [0, 1])
def test_long_row_list(dev, dtwin, extra):
    """As many long rows as the list holds, and one more: the row that finds the list full is hashed and inserted by its
    own wave -- the same codes.  Every third long row repeats an earlier one."""
    n = LONG_CAP + extra
    values = []
    for k in range(n):
        j = k - 2 if k % 3 == 2 else k
        values += [b"%06d" % j + bytes([65 + j % 26]) * (LONG_ROW - 5 + j % 9), b"s%d" % (k % 5)]
    want, _ = check(dev, dtwin, tdc.column_of(values), layouts=(False,), where=extra)
    assert sum(len(v) > LONG_ROW for v in values) == n
    tdc.check(want, values, int(want.res.flags))


def test_capacities(dev, dtwin):
    """The dictionary one entry short, its bytes one short, no room at all and more than enough: MSJ_CAPACITY where it
    is clipped, the codes complete, n_distinct and dict_bytes exact, nothing past the capacities written."""
    values = [b"v%d" % (k % 300) * (1 + k % 4) for k in range(2000)] + [bytes([66]) * 700, b"", None, bytes([66]) * 700]
    col = tdc.column_of(values)
    a = OnDevice(dev, col)
    full = tdc.twin_dictionary(dtwin, col)
    n, total = int(full.res.n_distinct), int(full.res.dict_bytes)
    tdc.check(full, values, int(full.res.flags))
    for cap, room in ((n - 1, total), (n, total - 1), (n - 1, total - 1), (0, 0), (1, 1), (n + 3, total + 9), (n, 0), (0, total), (B, total)):
        for flags in (0, WEAK):
            want = tdc.twin_dictionary(dtwin, col, flags=flags, dict_capacity=cap, dict_bytes_capacity=room)
            assert want.res.code == (MSJ_CAPACITY if cap < n or room < total else 0)
            same(device_dictionary(dev, a, want, shift=(cap + room) % 16), want, (cap, room, flags))


def test_rows_on_the_device(dev, dtwin):
    """d_n_rows equal to, below and above `rows`: below leaves the codes past R alone; above is MSJ_CAPACITY with n_rows =
    R and nothing else written; 0 writes d_dict_offsets[0] and a zero result."""
    values = [b"k%d" % (k % 19) if k % 5 else None for k in range(3 * B + 7)]
    col = tdc.column_of(values)
    a = OnDevice(dev, col)
    for R in (col.rows, col.rows - 1, B, 1, 0):
        want, _ = check(dev, dtwin, col, a=a, n_rows=R, where=R)
        tdc.check(want, values[:R], int(want.res.flags))
    for R in (col.rows + 1, 1 << 31, (1 << 64) - 1):
        want, got = check(dev, dtwin, col, a=a, n_rows=R, dict_capacity=5, dict_bytes_capacity=50, where=R)
        assert want.summary() == (MSJ_CAPACITY, 0, R, 0, 0, 0) and got.untouched(-1, 0, 0) and got.res.max_probe == 0


def test_hostile_offsets(dev, dtwin):
    """Offsets that descend, lie past bytes_len or are huge, and valid bytes other than 0 / 1, over more than one block:
    every such row is null, every other row keeps its value."""
    rng = np.random.default_rng(13)
    values = [b"w%d" % (k % 23) for k in range(2 * B + 40)]
    col = tdc.column_of(values)
    off = col.offsets.copy()
    for k in rng.integers(1, off.size - 1, 60):
        off[k] = [0, int(col.data.size) + 1 + int(k), (1 << 64) - 1, int(off[k - 1]), int(rng.integers(0, col.data.size))][int(k) % 5]
    valid = col.valid.copy()
    valid[::9] = rng.integers(0, 256, valid[::9].size)
    bad = tdc.Column(off, valid, col.data.tobytes())
    want, _ = check(dev, dtwin, bad, flags=(0, WEAK))
    tdc.check(want, bad.values(), int(want.res.flags))
    assert 0 < want.res.n_values < bad.rows


def test_bad_arguments(dev):
    """Each is refused with nothing launched, in the header's order: the outputs keep what was in them."""
    import torch

    col = tdc.column_of([b"a", b"b", b"a"])
    a = OnDevice(dev, col)
    sent = torch.full((8,), tvd.SENTINEL, dtype=torch.int64, device=dev.device)
    codes = torch.full((8,), 0x5A5A5A5A, dtype=torch.int32, device=dev.device)
    d_off = torch.full((8,), tvd.SENTINEL, dtype=torch.int64, device=dev.device)
    d_first = torch.full((8,), 0x5A5A5A5A, dtype=torch.int32, device=dev.device)
    out = torch.full((32,), 0x5A, dtype=torch.uint8, device=dev.device)
    n_rows = torch.full((2,), 3, dtype=torch.int64, device=dev.device)

    def call(**kw):
        p = dict(off=a.d_offsets.data_ptr(), val=a.d_valid.data_ptr(), rows=3, n_rows=n_rows.data_ptr(), data=a.d_bytes.data_ptr(), len=a.bytes_len,
                 codes=codes.data_ptr(), d_off=d_off.data_ptr(), d_first=d_first.data_ptr(), cap=4, out=out.data_ptr(), room=16, flags=0,
                 res=sent.data_ptr())
        p.update(kw)
        return dev.lib.msj_dictionary_device(dev.ctx, p["off"], p["val"], p["rows"], p["n_rows"], p["data"], p["len"], p["codes"], p["d_off"],
                                             p["d_first"], p["cap"], p["out"], p["room"], p["flags"], p["res"], dev._stream())

    assert dev.lib.msj_dictionary_device(None, *[None] * 2, 0, *[None] * 2, 0, *[None] * 3, 0, None, 0, 0, sent.data_ptr(), None) == BAD_ARGUMENT
    for name in ("res", "off", "val", "codes", "data", "d_off", "d_first", "out"):
        assert call(**{name: None}) == BAD_ARGUMENT, name
    assert call(flags=2) == BAD_ARGUMENT and call(flags=3) == BAD_ARGUMENT
    for name, base, step in (("off", a.d_offsets, 4), ("n_rows", n_rows, 4), ("d_off", d_off, 4), ("res", sent, 4), ("codes", codes, 2),
                             ("d_first", d_first, 1)):
        assert call(**{name: base.data_ptr() + step}) == BAD_ARGUMENT, name
    torch.cuda.synchronize()
    assert bool((sent == tvd.SENTINEL).all()) and bool((d_off == tvd.SENTINEL).all()) and bool((out == 0x5A).all())
    assert bool((codes == 0x5A5A5A5A).all()) and bool((d_first == 0x5A5A5A5A).all())
    ws = dev.lib.msj_dictionary_workspace_bytes
    assert ws(0) >= 4 * tdc.MIN_SLOTS and ws(1000) >= ws(0) + 12 * 1000 and ws(1 << 20) >= 12 * (1 << 20) + 4 * (2 << 20)
    # an unaligned d_dict_bytes, d_n_rows NULL, the layout-only form, and no row at all with NULL arrays
    assert call(out=out.data_ptr() + 3, room=8, n_rows=None) == 0
    torch.cuda.synchronize()
    assert out.cpu().numpy()[3:6].tobytes() == b"ab\x5a" and codes.cpu().numpy()[:4].tolist() == [0, 1, 0, 0x5A5A5A5A]
    assert d_off.cpu().numpy()[:3].tolist() == [0, 1, 2] and d_first.cpu().numpy()[:3].tolist() == [0, 1, 0x5A5A5A5A]
    assert sent.cpu().numpy()[:5].tolist() == [0, 3, 3, 2, 2]
    assert call(d_off=None, d_first=None, cap=0, out=None, room=0, flags=1) == 0
    torch.cuda.synchronize()
    assert sent.cpu().numpy()[:5].tolist() == [1 << 32, 3, 3, 2, 2]   # code 0, flags 1
    assert call(off=None, val=None, codes=None, rows=0, n_rows=None, data=None, len=0) == 0
    torch.cuda.synchronize()
    assert sent.cpu().numpy().tolist()[:6] == [0, 0, 0, 0, 0, 0] and d_off.cpu().numpy()[0] == 0


# ---- end to end -------------------------------------------------------------------------------------------------------------

def test_document_stream_categories(dev):
    """DocumentStream(select=[...]) over more than one window: Window.categories, ListColumn.categories,
    ElementFields.categories and MapColumn.key_categories against dict.setdefault over json.loads; Window.entries("")
    .schema() against the key sets and value kinds of json.loads; Window.raw(compact=True) into the dictionary: equal
    sub-objects written with different blanks get one code."""
    import torch
    from mojo_simdjson_amd.document_stream import DictionaryColumn, DocumentStream

    status = ["active", "suspended", "closed", "", "actíve"]
    docs = [{"id": k, "status": status[(k * k) % 5], "tags": ["t%d" % (k % 4), k, "t%d" % (k % 3)], "attrs": {"color": "c%d" % (k % 3), "n%d" % (k % 6): k},
             "items": [{"sku": "s%d" % ((k + j) % 4), "q": j} for j in range(k % 3)], "geo": {"lat": (k // 2) % 2, "lon": [k % 3]}} for k in range(150)]
    docs[7] = {"id": "seven", "status": 5, "tags": 5, "extra": None, "geo": "nowhere"}
    docs[11] = {"status": "active"}   # (written with an escape below: the same value)
    lines = [json.dumps(d, indent=None if k % 2 else 2, ensure_ascii=False).encode() for k, d in enumerate(docs)]
    lines[11] = b'{"status":"act\\u0069ve"}'
    data = b"\n".join(lines) + b"\n"
    pointers = ["", "/status", "/tags", "/attrs", "/items", "/geo"]
    tag = lambda v: "n" if v is None else "t" if v is True else "f" if v is False else "l" if isinstance(v, int) else \
        "d" if isinstance(v, float) else '"' if isinstance(v, str) else "[" if isinstance(v, list) else "{"

    def agree(cats, values, what):
        assert isinstance(cats, DictionaryColumn) and cats.codes.dtype == torch.int32 and cats.codes.is_cuda and cats.bytes.is_cuda, what
        codes, distinct, first = tdc.definition([v.encode() if isinstance(v, str) else None for v in values])
        got_values, got_codes = cats.to_python()
        assert got_codes == codes and got_values == [v.decode() for v in distinct] and cats.first.cpu().tolist() == first, what
        assert cats.counts().cpu().tolist() == [codes.count(c) for c in range(len(distinct))] and cats.n_distinct == len(distinct), what

    seen = windows = 0
    for win in DocumentStream(dev, tvd.upload(dev, data), len(data), window=8192, select=pointers):
        D = win.n_documents
        mine = docs[seen:seen + D]
        agree(win.categories("/status"), [d.get("status") for d in mine], "status")
        tags = win.elements("/tags")
        agree(tags.categories(), [x for d in mine if isinstance(d.get("tags"), list) for x in d["tags"]], "tags")
        items = win.elements("/items").select(["/sku"])
        agree(items.categories("/sku"), [x["sku"] for d in mine for x in d.get("items", [])], "sku")
        attrs = win.entries("/attrs")
        agree(attrs.key_categories(), [key for d in mine for key in d.get("attrs", {})], "attrs")
        roots = win.entries("")
        want = {}
        for d in mine:
            for key, v in d.items():
                entry = want.setdefault(key, [0, set()])
                entry[0] += 1
                entry[1].add(tag(v))
        schema = roots.schema()
        assert [name for name, _, _ in schema] == list(want) and {name: [n, kinds] for name, n, kinds in schema} == want
        # equal sub-objects with different blanks: one code in the compact form, and the codes of json.loads' values
        offsets, raw, valid = win.raw("/geo", compact=True)
        res, d_codes, *_ = dev.dictionary(offsets, raw, valid.view(torch.uint8), rows=D)
        geo = [json.dumps(d["geo"], separators=(",", ":")) if "geo" in d else None for d in mine]
        codes, distinct, _ = tdc.definition([g.encode() if g is not None else None for g in geo])
        assert d_codes[:D].cpu().tolist() == codes and res.n_distinct == len(distinct) <= 7
        v_offsets, v_raw, v_valid = win.raw("/geo")
        verbatim, *_ = dev.dictionary(v_offsets, v_raw, v_valid.view(torch.uint8), rows=D, values=False)
        assert verbatim.n_distinct >= res.n_distinct and (D < 24 or verbatim.n_distinct > res.n_distinct)
        seen += D
        windows += 1
    assert windows >= 2 and seen == len(docs)
