"""The corpus and the expected values of tests/test_stale_tails.py: windows whose counts leave every kernel's last unit
partly filled, and three states of what lies behind those counts in arrays that a longer window has used -- all on the
CPU, from the oracles and the host twins (tests/stream_order.py: Expected), never from a device.

The product allocates every array behind stage 1 once, at capacity size, and never clears it (DocumentStream): a short
window that follows a long one has the long one's tokens, flags, partners, number records and rows behind its own counts,
and nothing but a guard such as `t < nrem` or `k < h.R` stands between a kernel and them.

The windows.  Window r is the first k lines of window A (so.lines_a()) and one tuning line behind them: document 601 of A's
shape with m more scalars in its "tags".  A scalar element is two tokens (itself and its comma) whatever its kind, so the
parity is set by one empty array, three tokens, where it has to change.  k sets the document count D = k + 1, m the token
count n: n mod 4096 = r for every r of REMAINDERS.  The units that these phases fill to "one item" and "one short":

    the tokens kernels' and the documents kernel's block   2 048 tokens, 8 per thread, rows of 64     (tokens_kernel.hip, documents_kernel.hip: kBlock, kPer)
    the span kernels                                           512 tokens, 2 per thread; chunks of 128  (kSpanTokens, kSpanPer, kChunk)
    the numbers kernel                                       4 096 tokens, 16 flags per thread, read 8 at a time  (numbers_kernel.hip: kBlock, kPer)
    the verdict kernels                                      1 024 tokens, groups of 4 type bytes      (validate_block.h: kBlock, kPer)
    the column kernels                                         256 rows, four waves of 64              (rows_block.h: kRowBlock)

Every token unit divides 4 096, so the remainders 1 and 4 095 put all of them at one item and at one short at once; 2 047 ..
2 049 do the same for the units up to 2 048 from the other side of a block border.  D mod 256 takes 0, 1 and 255 and D mod 64
takes 1 and 63 (DOCUMENTS).  The other counts -- numbers, items, entries, bytes -- fall where they fall and are printed.

The stale states (STATES), each a full image of every array of the chain at the size of the larger of A and B plus SLACK
elements, so that a block-wide read or write behind a window's counts stays inside the tensor:

    poison         a table, one pattern per array, that does the most damage to a reader that ignores its bound AND is in
                   bounds of every allocation whatever it is used as: types are brackets and quotes in turn (TYPES), flags 0xFF,
                   depths 0, partners / first tokens / the token fields of records are tokens below the smallest window's n,
                   idx and end are offsets inside the buffer, offsets are 0, valid is 1
    decoy          the poison with what the chain over window B writes laid over it: behind the window's counts lie the
                   valid-looking tokens of another stream of A's sizes
    continuation   the poison with what the chain over all of A writes laid over it: behind n lies the stream's true next
                   document, as in DocumentStream

No state holds an array's fill where a value could be used as an index: what lies behind A's own extents is the poison.

What a call writes is taken from the twin's array (`written`): an element of 4, 8, 16 or 32 bytes is untouched iff all of
its bytes are the array's fill; the text arrays (FILL 0x77 is the letter w) are written over the prefix that the twin's
result counts (the tape's string buffer: but for the slots of invalid documents, `string_slots`), type / flags / valid
over their first n or R bytes.  The CPU test holds these masks against the counted
extents (`extents`), so that no position accepts two values.
"""
import functools

import numpy as np

from mojo_simdjson_amd.document_stream import FIELD_DTYPE
from tests import helpers
from tests import stream_order as so
from tests import test_validate_documents_math as tdm

REMAINDERS = (0, 1, 2, 3, 7, 9, 15, 17, 63, 65, 2047, 2048, 2049, 4095)
PHASE = 4096             # the largest unit: the numbers kernel's block
# remainder -> D: mod 256 in {0, 1, 255} at the block borders and the extremes, mod 64 in {1, 63} elsewhere
DOCUMENTS = {0: 256, 1: 257, 2: 65, 3: 63, 7: 129, 9: 127, 15: 193, 17: 191, 63: 385, 65: 319, 2047: 511, 2048: 512, 2049: 513, 4095: 255}
TUNING = 601             # the tuning line's document number: odd, so that it has items
SLACK = 4096             # elements behind the larger of A's and B's arrays
STATES = ("decoy", "continuation", "poison")

WIDTH = {"idx": 4, "type": 1, "depth": 4, "match": 4, "end": 4, "flags": 1, "first": 4, "records": 16, "rows": 16, "tape": 8, "sbuf": 1,
         "recs": 32, "fields": 16, "offsets": 8, "valid": 1, "data": 1, "elements": 16, "keys": 16, "values": 16, "codes": 4,
         "dict_offsets": 8, "dict_first": 4, "dict_bytes": 1}
TEXT = ("sbuf", "data", "dict_bytes")       # written over a counted prefix; the fill occurs in the data
BYTES = ("type", "flags", "valid")          # written over their first n or R bytes
# the poison's type bytes: of any two neighbours one is a closing bracket, and they outnumber the opening ones, so that a
# depth pass that reads even one of them behind a stream that ends at depth 0 reports a minimum below 0
TYPES = b']"}['


# ---- the windows ------------------------------------------------------------------------------------------------------------

def tuning_line(m, odd):
    """Document TUNING of A's shape with m more scalars in its tags (numbers, strings and literals in turn) and, odd, one
    empty array behind them"""
    doc = so.document_a(TUNING)
    doc["tags"] += [(j, "e%d" % j, j % 2 == 0, None)[j % 4] for j in range(m)] + [[]] * odd
    return so.line(TUNING, doc)


def count_tokens(text):
    code, n, _ = helpers.run_oracle(so.twins().oracle.msj_oracle_stage1, text)
    assert code == 0
    return n


@functools.lru_cache(maxsize=None)
def window_lines(r):
    """The lines of window r: (k, m) by search on the CPU -- k from DOCUMENTS, m the extra scalars with n mod PHASE == r"""
    a = so.expected("A")
    k = DOCUMENTS[r] - 1
    in_front = int(a.w.first[k])                   # the tokens of A's first k lines
    for odd in (0, 1):
        # (the search starts where two tokens per scalar and three per empty array put the answer, and counts what it finds)
        short = (r - in_front - count_tokens(tuning_line(0, odd))) % PHASE
        for m in (short // 2, short // 2 + 1):
            text = tuning_line(m, odd)
            if (in_front + count_tokens(text)) % PHASE == r:
                return a.lines[:k] + [text]
    raise AssertionError(f"no tuning line for remainder {r}")


@functools.lru_cache(maxsize=None)
def expected(r):
    return so.Expected.from_lines(f"S{r}", window_lines(r))


# ---- what a call writes -----------------------------------------------------------------------------------------------------

def string_slots(x):
    """The tape's string buffer is no counted prefix: a document with a verdict code keeps its slot [string_first[k],
    string_first[k + 1]), whose contents are unspecified (include/msj_stage1.h: msj_tape_documents_device) -- the twin and
    the kernel both leave it alone, so it belongs to what stays as it was.  -> the slots of the documents that are built"""
    recs = x.tape.recs[:x.D]
    edges = [int(v) for v in recs["string_first"]] + [int(x.tape.res.string_bytes)]
    out = []
    for k in range(x.D):
        if int(recs["code"][k]) == 0 and edges[k] < edges[k + 1]:
            if out and out[-1][1] == edges[k]:
                out[-1] = (out[-1][0], edges[k + 1])
            else:
                out.append((edges[k], edges[k + 1]))
    return out


def extents(x):
    """{(call, array): [(lo, hi)] in elements (bytes for the text and byte arrays)}: what the window's counts say each call
    of the chain writes"""
    n, D, rows, erows, E = x.n, x.D, x.rows, x.erows, x.E
    out = {("shard", "idx"): [(0, n)], ("documents", "first"): [(0, D)], ("number_values", "records"): [(0, x.ncap)],
           ("validate_documents", "rows"): [(0, D)], ("tape_documents", "tape"): [(0, int(x.tape.res.tape_words))],
           ("tape_documents", "sbuf"): string_slots(x), ("tape_documents", "recs"): [(0, D)],
           ("select_documents", "fields"): [(p * rows, p * rows + D) for p in range(len(so.POINTERS))],
           ("select_elements", "fields"): [(p * erows, p * erows + E) for p in range(len(so.ELEMENT_POINTERS))]}
    for name in ("type", "depth", "match", "end", "flags"):
        out["stage2_prep", name] = [(0, n)]
    for call, c, R in (("string_column", x.strings, D), ("array_column", x.lists, D), ("array_elements", x.sublists, E), ("object_entries", x.maps, D),
                       ("raw_column", x.raw[False], D), ("raw_column_compact", x.raw[True], D)):
        assert int(c.res.n_rows) == R
        out[call, "offsets"], out[call, "valid"] = [(0, R + 1)], [(0, R)]
    for call, c in (("string_column", x.strings), ("raw_column", x.raw[False]), ("raw_column_compact", x.raw[True])):
        out[call, "data"] = [(0, int(c.res.total_bytes))]
    out["array_column", "elements"] = [(0, int(x.lists.res.n_elements))]
    out["array_elements", "elements"] = [(0, int(x.sublists.res.n_elements))]
    out["object_entries", "keys"] = out["object_entries", "values"] = [(0, int(x.maps.res.n_entries))]
    for call, e in (("dictionary_strings", x.dict_strings), ("dictionary_raw", x.dict_raw)):
        distinct = int(e.res.n_distinct)
        out[call, "codes"], out[call, "dict_offsets"] = [(0, int(e.res.n_rows))], [(0, distinct + 1)]
        out[call, "dict_first"], out[call, "dict_bytes"] = [(0, distinct)], [(0, int(e.res.dict_bytes))]
    return out


def written(x, call, o, ext=None):
    """The bytes of o.want that the call writes, a bool per byte (see the module's text)"""
    width = WIDTH[o.name]
    if o.name in TEXT or o.name in BYTES:
        mask = np.zeros(o.want.size, dtype=bool)
        for lo, hi in (ext or extents(x))[call, o.name]:
            mask[lo:hi] = True
        return mask
    whole = o.want.size // width * width          # (a canary is a whole number of elements everywhere: asserted on the CPU)
    mask = np.zeros(o.want.size, dtype=bool)
    mask[:whole] = np.repeat((o.want[:whole].reshape(-1, width) != o.fill).any(axis=1), width)
    return mask


def arrays(x):
    """(call, Out) of every output array of the chain, the result structs left out"""
    return [(call, o) for call, outs in x.calls.items() for o in outs if o.struct is None]


# ---- the tensors' sizes and the stale states -----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def sizes():
    """{(call, array): bytes of the one tensor that serves every window}: the larger of A's and B's, plus SLACK elements;
    a result struct has its own size"""
    a, b = so.expected("A"), so.expected("B")
    out = {}
    for call, outs in a.calls.items():
        for o, ob in zip(outs, b.calls[call]):
            slack = 0 if o.struct is not None else SLACK * WIDTH[o.name]
            out[call, o.name] = max(o.want.size, ob.want.size) + slack
    return out


def buffer_length():
    """The bytes of d_buf: A's length (B's is the same)"""
    return so.expected("A").length


def window_bytes(x):
    """What d_buf holds for the window x: its bytes, B's behind them up to A's length.  The calls get len(x.data)."""
    b = so.expected("B").data
    assert len(x.data) <= len(b)
    return x.data + b[len(x.data):]


@functools.lru_cache(maxsize=None)
def poison_tokens():
    """The poison's token numbers lie below this: the smallest window's n"""
    return min(expected(r).n for r in REMAINDERS)


def poison(name, size):
    """The poison of the array `name` over `size` bytes (see the module's text)"""
    tokens, length = poison_tokens(), buffer_length()
    count = size // WIDTH[name]
    i = np.arange(count, dtype=np.uint64)
    token = ((i * np.uint64(7) + np.uint64(3)) % np.uint64(tokens)).astype(np.uint32)
    if name == "type":
        out = np.frombuffer(TYPES, dtype=np.uint8)[np.arange(count) % len(TYPES)]
    elif name == "flags":
        out = np.full(count, 0xFF, dtype=np.uint8)
    elif name in ("depth", "offsets", "dict_offsets", "codes", "dict_first"):
        out = np.zeros(size, dtype=np.uint8)
    elif name == "valid":
        out = np.ones(count, dtype=np.uint8)
    elif name in ("match", "first"):
        out = token
    elif name in ("idx", "end"):
        out = ((i * np.uint64(13) + np.uint64(1)) % np.uint64(length)).astype(np.uint32)
    elif name == "records":
        out = np.zeros(count, dtype=tdm.NUMBER_DTYPE)
        out["bits"], out["token"], out["kind"] = i, token, 1
    elif name == "rows":
        out = np.zeros(count, dtype=tdm.VERDICT_DTYPE)
        out["error_token"] = token
    elif name in ("fields", "elements", "keys", "values"):
        # strings of 8 bytes inside the window, arrays and objects that close on a later token below n, in turn: live rows
        out = np.zeros(count, dtype=FIELD_DTYPE)
        kind = np.arange(count) % 3
        out["token"], out["type"] = token, np.frombuffer(b'"[{', dtype=np.uint8)[kind]
        span = (np.uint64(1) + i % np.uint64(1000)) | (np.uint64(8) << np.uint64(32))
        out["bits"] = np.where(kind == 0, span, np.minimum(token.astype(np.uint64) + np.uint64(5), np.uint64(tokens - 1)))
    elif name in TEXT:
        out = np.full(count, ord("p"), dtype=np.uint8)
    else:   # tape, recs: no call reads them
        out = np.full(size, 0x3C, dtype=np.uint8)
    out = np.ascontiguousarray(out).view(np.uint8).reshape(-1)
    return np.concatenate([out, np.full(size - out.size, 0x3C, dtype=np.uint8)])


@functools.lru_cache(maxsize=None)
def stale(state):
    """{(call, array): the state's bytes over the whole tensor}.  The result structs: B's, A's, zeros."""
    assert state in STATES
    src = {"decoy": so.expected("B"), "continuation": so.expected("A"), "poison": None}[state]
    out = {}
    for (call, name), size in sizes().items():
        if name not in WIDTH:
            out[call, name] = np.zeros(size, dtype=np.uint8)
        else:
            out[call, name] = poison(name, size)
    if src is not None:
        ext = extents(src)
        for call, outs in src.calls.items():
            for o in outs:
                full = out[call, o.name]
                if o.struct is not None:
                    full[:] = o.want
                    continue
                mask = written(src, call, o, ext)
                full[:o.want.size][mask] = o.want[mask]
    for full in out.values():
        full.setflags(write=False)
    return out


def full_want(x, state):
    """{(call, array): (the bytes the whole tensor holds behind the window's chain over the state, how many of them are
    compared)}: the twin's where the call writes, the state's everywhere else.  Stage 1 leaves a trailer behind its indices
    that no caller may read (so.Out.upto): the first n are compared."""
    ext, before, out = extents(x), stale(state), {}
    for call, o in arrays(x):
        full = before[call, o.name].copy()
        mask = written(x, call, o, ext)
        full[:o.want.size][mask] = o.want[mask]
        out[call, o.name] = (full, full.size if o.upto is None else o.upto)
    return out


def out_of_bounds(state):
    """Every value of the state that a kernel could use as an index or an offset, against the test's own allocations ->
    [(call, array, what)] of those that are not below them (empty: a kernel that wrongly uses one shows a wrong array,
    never a fault)"""
    s, size, length, bad = stale(state), sizes(), buffer_length(), []
    tokens = min(size["stage2_prep", name] // WIDTH[name] for name in ("type", "depth", "match", "end", "flags")) - SLACK
    none = 0xFFFFFFFF

    def below(key, what, values, bound, sentinel=False):
        values = np.asarray(values).astype(np.uint64).reshape(-1)
        if sentinel:   # "none", in 32 or in 64 bits
            values = values[(values != none) & (values != 0xFFFFFFFFFFFFFFFF)]
        if values.size and int(values.max()) >= bound:
            bad.append(key + (what, int(values.max()), bound))

    for key, raw in s.items():
        call, name = key
        if name in ("idx", "end"):
            below(key, "offset", raw.view(np.uint32), length + 1)          # (an end is the offset behind a token's last byte)
        elif name == "match":
            below(key, "token", raw.view(np.uint32), tokens, sentinel=True)
        elif name == "first":
            below(key, "token", raw.view(np.uint32), tokens)
        elif name == "records":
            below(key, "token", raw[:raw.size // 16 * 16].view(tdm.NUMBER_DTYPE)["token"], tokens)
        elif name == "rows":
            below(key, "token", raw[:raw.size // 16 * 16].view(tdm.VERDICT_DTYPE)["error_token"], tokens + 1, sentinel=True)
        elif name in ("fields", "elements", "keys", "values"):
            f = raw[:raw.size // 16 * 16].view(FIELD_DTYPE)
            below(key, "token", f["token"], tokens, sentinel=True)
            strings, containers = f["type"] == ord('"'), np.isin(f["type"], np.frombuffer(b"[{", dtype=np.uint8))
            below(key, "span", (f["bits"][strings] & np.uint64(none)) + (f["bits"][strings] >> np.uint64(32)), length + 1)
            below(key, "partner", f["bits"][containers], tokens)
        elif name in ("offsets", "dict_offsets"):
            data = {"dict_offsets": "dict_bytes"}.get(name, "data")
            bound = size[call, data] if (call, data) in size else min(size[call, e] // 16 for e in ("elements", "keys", "values") if (call, e) in size)
            below(key, "offset", raw[:raw.size // 8 * 8].view(np.uint64), bound + 1)
        elif name in ("codes", "dict_first"):
            rows = size[call, "codes"] // 4
            below(key, "row or code", raw[:raw.size // 4 * 4].view(np.uint32), rows, sentinel=True)
    return bad


# ---- the calls outside the chain ----------------------------------------------------------------------------------------------

OUTSIDE_STATES = ("decoy", "poison")
PAIR_DTYPE = np.dtype([("open", "<u4"), ("close", "<u4")])     # msj_bracket_pair


class TokenCalls:
    """What msj_tokens_chain_device, msj_token_spans_device, the two pairs calls and msj_depth_from_types_device leave for
    the window x, from oracle/tokens_oracle.c (helpers.oracle_tokens, oracle_match, oracle_token_spans), and the caller's
    arrays they run on: the chain's arrays of the same names in a stale state, the pairs like the partners."""

    def __init__(self, x):
        self.x, self.n = x, x.n
        idx = x.w.idx
        self.type, self.depth, (final, lo, hi) = helpers.oracle_tokens(x.data, idx)
        self.match = helpers.oracle_match(self.type)
        self.end, self.flags = helpers.oracle_token_spans(x.data, idx)
        opens = np.nonzero(np.isin(self.type, np.frombuffer(b"[{", dtype=np.uint8)))[0]
        self.pairs = np.zeros(opens.size, dtype=PAIR_DTYPE)
        self.pairs["open"], self.pairs["close"] = opens, self.match[opens]
        self.result = (x.n, final, lo, hi, int(opens.size))      # n, final / min / max depth, the opening brackets

    def want(self, name):
        return np.ascontiguousarray(getattr(self, name)).view(np.uint8).reshape(-1)

    def before(self, state, name):
        """The caller's array `name` in front of a call: the stale state of the chain's array of that name; the pairs: two
        partners' worth per record (tokens below n in the poison, B's or the poison's in the decoy)"""
        s = stale(state)
        if name == "idx":
            return s["shard", "idx"]
        if name == "pairs":
            return np.concatenate([s["stage2_prep", "match"]] * 2)
        return s["stage2_prep", name]

    def inputs(self, state, name):
        """An input array (idx, or depth_from_types' type): the window's own values, the stale tail behind them"""
        full = self.before(state, name).copy()
        mine = np.ascontiguousarray(self.x.w.idx if name == "idx" else self.type).view(np.uint8).reshape(-1)
        full[:mine.size] = mine
        return full

    def after(self, state, name):
        """The caller's array behind a call: the oracle's over [0, n) -- the pairs: over the opening brackets --, untouched behind"""
        full = self.before(state, name).copy()
        mine = self.want(name)
        full[:mine.size] = mine
        return full


@functools.lru_cache(maxsize=None)
def token_calls(r):
    return TokenCalls(expected(r))


class RowCalls:
    """msj_filter_rows_device, msj_take_rows_device and msj_cast_strings_device over the records that a stale run's
    select_documents leaves, with capacity = rows: the ROOM records behind the D of every path are the stale state's and
    look live.  All from the twins (tests/filter_rows_math_host.cpp, tests/cast_strings_math_host.cpp).  One predicate set --
    a number compare and a string equality, ALL; no path of so.POINTERS selects a number, so the compare is negated: it
    is evaluated on every row and holds on all of them -- and one cast of each kind over the column /status."""

    def __init__(self, x, state):
        from tests import test_cast_strings_math as tcs
        from tests import test_filter_rows_math as tfm

        self.specs = [tfm.Spec(so.P_STATUS, tfm.STR_EQ, b"active"), tfm.Spec(so.P_ITEMS, tfm.NUM_LT, 5, neg=True)]
        self.device_specs = [(so.P_STATUS, "==", "active"), ("not", (so.P_ITEMS, "<", 5))]
        ftwin, ctw = tfm.load_twin(), tcs.load_twin()
        n_paths, rows = len(so.POINTERS), x.rows
        full, _ = full_want(x, state)["select_documents", "fields"]
        records = full[:16 * n_paths * rows].view(FIELD_DTYPE)
        data = window_bytes(x)
        blob = tfm.compile_specs(ftwin, self.specs, False)
        f = self.filtered = tfm.twin_filter(ftwin, blob, data, x.length, records, rows, n_paths, x.sel.res, rows)
        assert f.rc == 0 and f.res.code == 0 and 0 < f.res.n_kept < x.D and f.res.n_rows == x.D
        self.taken, self.out, self.out_select = tfm.twin_take(ftwin, f.kept[:rows], f.kept_select, records, rows, n_paths, x.sel.res, rows, rows)
        assert self.taken.code == 0 and self.taken.n_rows == f.res.n_kept
        column = records[so.P_STATUS * rows:(so.P_STATUS + 1) * rows]
        self.casts = {kind: tcs.twin_cast(ctw, data, column, {"timestamp": tcs.TIMESTAMP, "number": tcs.NUMBER}[kind],
                                          "ms" if kind == "timestamp" else "s", 0, R=x.D,
                                          length=x.length, capacity=rows) for kind in ("timestamp", "number")}
        assert all(c.rc == 0 and c.res.code == 0 and c.res.n_rows == x.D for c in self.casts.values())

    def arrays(self):
        """{name: the expected bytes, fill and canary included}"""
        f = self.filtered
        struct = lambda s: np.frombuffer(bytes(s), dtype=np.uint8)
        out = {"keep": f.keep, "kept": f.kept.view(np.uint8), "res": struct(f.res), "ksel": struct(f.kept_select),
               "out": self.out.view(np.uint8).reshape(-1), "tres": struct(self.taken), "osel": struct(self.out_select)}
        for kind, c in self.casts.items():
            out.update({f"cast_{kind}": c.out, f"cres_{kind}": struct(c.res), f"csel_{kind}": struct(c.sel)})
        return out
