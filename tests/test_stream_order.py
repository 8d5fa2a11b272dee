"""The device calls behind stage 1 in stream order: on a side stream, behind an input that arrives late, many in flight, on
a context that other windows have used, on two contexts at once (include/msj_stage1.h: "all on the device, on the caller's
stream, no host round trip").

Every other GPU test of these calls runs on torch's current stream, the legacy null stream, where everything in the process
is ordered behind everything else: a launch or a hipMemsetAsync that dropped its stream, a helper tensor filled on another
stream or a result read with the wrong synchronisation passes there.  Here the whole chain of tests/stream_order.py is
enqueued with sync=False, every capacity given and every output a tensor of the caller's, and is held against the host
twins' expected values over the WHOLE arrays, fill and canary included -- never against another device run.

One set of tensors (Tensors) belongs to one window's expected values.  Its arrays are put back to their fill by copies
that are part of the chain, in stream order: a call that runs ahead of its stream therefore reads what the last chain left
-- a consistent, valid state -- and what it writes is then overwritten with the fill, so that it shows as a wrong array.
"""
import json
import time

import numpy as np
import pytest

from mojo_simdjson_amd import _lib
from tests import stream_order as so
from tests import test_array_column_math as tac
from tests import test_dictionary_math as tdc
from tests import test_select_math as tsm
from tests import test_string_column as tsc
from tests import test_string_column_math as tcm
from tests import test_tape_documents as ttd
from tests import test_tape_documents_math as tdk
from tests import test_validate_documents as tvd

WINDOW = 8192            # test_document_stream_on_a_side_stream: windows of the fewest multiples of 8 KiB that hold A's longest document
MIN_DELAY_MS = 50.0      # the late input is at least this late, and at least JITTER times the host side of an enqueue
JITTER = 20
SLEEP_UNIT = 2_000_000   # cycles of torch.cuda._sleep: the first unit timed to size the delay (x 8 until it lasts 2 ms)
SMALL_LIMITS = (4096, 3)  # msj_debug_set_span_limits: the LDS limit and the fix-up list's capacity of tests/test_tokens.py


# ---- the corpus, on the CPU -----------------------------------------------------------------------------------------------------

def test_corpus_on_cpu():
    """The three windows are what the GPU tests need: A's sizes and special pieces, B equal to A in every size the host
    passes to a call, A's expected values equal to json.loads through the definitions of the calls' own CPU tests, and for
    EVERY call of the chain at least one output array that differs between A and B."""
    a, b, c = so.expected("A"), so.expected("B"), so.expected("C")
    for x in (a, b, c):
        print(f"window {x.name}: {x.length} bytes, {x.n} tokens, {x.D} documents, {x.ncap} numbers, {x.E} items, "
              f"{int(x.maps.res.n_entries)} entries, {int(x.dict_strings.res.n_distinct)} distinct strings")
    assert (a.length, a.n, a.D, a.ncap) == (b.length, b.n, b.D, b.ncap) and a.data != b.data
    assert a.D == so.A_DOCS > 2 * 256 and 20000 <= a.n <= 40000 and (128 << 10) <= a.length <= (512 << 10)
    assert a.E > 256 and c.D == so.C_DOCS and c.n < a.n and c.length < a.length
    assert all(x.vres.code == 0 and x.tape.res.code == 0 and x.sel.res.code == 0 for x in (a, b, c))

    # the pieces that reach the device-only paths
    w = a.w
    size = w.end.astype(np.int64) - w.idx.astype(np.int64)
    is_string, is_number = w.typ == ord('"'), (w.flags & 4) != 0
    escaped = is_string & ((w.flags & tcm.ESCAPED) != 0)
    assert int((escaped & (size - 1 > 1024)).sum()) >= 4 and int((escaped & (size - 1 > 4096)).sum()) >= 1
    assert int((is_number & (size > 64)).sum()) == 1
    lengths = np.diff(a.strings.offsets[:a.D + 1].astype(np.int64))
    codes = a.dict_strings.codes
    assert int((lengths > 512).sum()) >= 3 and codes[so.EQUAL_LONG[0]] == codes[so.EQUAL_LONG[1]] != codes[so.OTHER_LONG]
    assert all(lengths[k] > 512 for k in so.EQUAL_LONG + (so.OTHER_LONG,))
    assert int(np.diff(a.raw[False].offsets[:a.D + 1].astype(np.int64)).max()) > 16384
    assert [k for k, code in enumerate(a.codes) if code] == [so.INVALID]
    assert a.sel.column(2)[so.MISSING]["code"] == 20 and a.sel.column(2)[so.INVALID]["code"] == a.codes[so.INVALID]

    # A's expected values are json.loads', through the definitions the calls' own CPU tests use
    t = so.twins()
    values = tsm.check_against_reference(w, a.sel, so.POINTERS, a.lines, codes=a.codes)
    column = lambda p: [values[(p, k)] for k in range(a.D)]
    tdk.check_against_definition(t.tm, w, a.tape, codes=a.codes, texts=a.lines)
    tcm.check_against_definition(a.strings, column(so.P_STATUS), a.sel.column(so.P_STATUS)[:a.D])
    tac.check_against_definition(w, a.lists, column(so.P_ITEMS))
    docs = [None if code else json.loads(text) for code, text in zip(a.codes, a.lines)]
    status = [d["status"].encode() if d is not None else None for d in docs]
    tdc.check(a.dict_strings, status)
    geo = [json.dumps(d["geo"], separators=(",", ":")).encode() if d is not None and "geo" in d else None for d in docs]
    assert a.raw[True].rows() == geo and [r and json.loads(r) for r in a.raw[False].rows()] == [g and json.loads(g) for g in geo]
    tdc.check(a.dict_raw, geo)

    # a call that runs on the decoy's state gives other arrays than A's: every call, or the corpus has to change
    table = so.differing(a, b)
    for call, names in table.items():
        print(f"A differs from B in {call}: {', '.join(names) or 'NOTHING'}")
    assert all(table.values()) and list(table) == list(a.calls)


# ---- the chain on the device ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def dev():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mojo_simdjson_amd.device import Stage1Device

    d = Stage1Device(0)
    yield d
    d.close()


class Context:
    """A Stage1Device with the two path lists compiled for it"""

    def __init__(self, dev=None):
        from mojo_simdjson_amd.device import Stage1Device

        self.owned = dev is None
        self.dev = Stage1Device(0) if dev is None else dev
        env = tsc.Env(self.dev)
        self.paths, self.epaths = env.paths(so.POINTERS), env.paths(so.ELEMENT_POINTERS)

    def close(self):
        if self.owned:
            self.dev.close()


class Tensors:
    """The tensors one chain over the window `x` (so.Expected) writes: one per output array of every call, uint8, of the
    twin's size, and beside each a copy that keeps the call's fill"""

    def __init__(self, dev, x):
        self.x, self.t, self.pristine = x, {}, {}
        for call, outs in x.calls.items():
            for o in outs:
                fill = np.full(o.want.size, o.fill, dtype=np.uint8)
                self.t[call, o.name], self.pristine[call, o.name] = ttd.to_device(dev, fill), ttd.to_device(dev, fill)
        self.zero = dev.new_carry()

    def refill(self):
        """Every array back to its fill, on the current stream"""
        for key, d in self.t.items():
            d.copy_(self.pristine[key], non_blocking=True)

    def u8(self, call, name):
        return self.t[call, name]

    def i32(self, call, name):
        import torch

        return self.t[call, name].view(torch.int32)

    def i64(self, call, name):
        import torch

        return self.t[call, name].view(torch.int64)

    def records(self, call, name, width=2):
        return self.i64(call, name).view(-1, width)


def chain(c, d_buf, t, refill=True):
    """The whole chain over the window in d_buf into the tensors t: nothing is read back, nothing is sized from a first
    call.  A generator that stops behind every call (its name), so that two chains can be enqueued in turns.  refill False:
    the arrays keep what they hold (tests/test_stale_tails.py puts a larger window's leftovers there)."""
    dev, x = c.dev, t.x
    n, L, rows, erows, ncap = x.n, x.length, x.rows, x.erows, x.ncap
    if refill:
        t.refill()
    yield "fill"
    d_idx, d_carry = t.i32("shard", "idx"), t.u8("shard", "carry")
    dev.shard(d_buf, L, d_idx, t.zero, d_carry, is_final=False)
    yield "shard"
    arrays = (t.u8("stage2_prep", "type"), t.i32("stage2_prep", "depth"), t.i32("stage2_prep", "match"), t.i32("stage2_prep", "end"),
              t.u8("stage2_prep", "flags"))
    d_type, d_depth, _, d_match, d_end, d_flags = dev.stage2_prep(d_buf, L, d_idx, n, d_result=t.u8("stage2_prep", "res"), arrays=arrays, sync=False)
    yield "stage2_prep"
    d_first, d_docs = t.i32("documents", "first")[:rows], t.u8("documents", "res")
    dev.documents(d_buf, L, d_idx, n, d_type, d_depth, is_final=False, d_carry=d_carry, d_doc_first=d_first, d_result=d_docs, sync=False)
    yield "documents"
    d_numbers, d_num = t.records("number_values", "records"), t.u8("number_values", "res")
    dev.number_values(d_buf, L, d_idx, n, d_flags, capacity=ncap, d_result=d_num, sync=False, d_numbers=d_numbers)
    yield "number_values"
    tokens = (d_idx, n, d_type, d_depth, d_match, d_end, d_flags)
    numbers = dict(d_numbers=d_numbers, numbers_capacity=ncap, d_numbers_result=d_num)
    d_verdicts = t.records("validate_documents", "rows")
    dev.validate_documents(d_buf, L, *tokens, d_first, d_docs, max_depth=100, d_verdicts=d_verdicts, capacity=x.D,
                           d_result=t.u8("validate_documents", "res"), sync=False, **numbers)
    yield "validate_documents"
    caps = x.tape.caps
    dev.tape_documents(d_buf, L, *tokens, d_first, d_docs, d_numbers, caps["numbers_capacity"], d_verdicts=d_verdicts,
                       d_tape=t.i64("tape_documents", "tape"), tape_capacity=caps["tape_capacity"], d_string_buf=t.u8("tape_documents", "sbuf"),
                       string_capacity=caps["string_capacity"], d_doc_tapes=t.records("tape_documents", "recs", 4), capacity=caps["capacity"],
                       d_result=t.u8("tape_documents", "res"), sync=False)
    yield "tape_documents"
    n_paths = len(so.POINTERS)
    d_fields, d_sel = t.records("select_documents", "fields")[:n_paths * rows].view(n_paths, rows, 2), t.u8("select_documents", "res")
    dev.select_documents(c.paths, d_buf, L, *tokens, d_first, d_docs, d_verdicts=d_verdicts, d_fields=d_fields, capacity=rows, d_result=d_sel,
                         sync=False, **numbers)
    yield "select_documents"
    column = lambda call, data: dict(d_offsets=t.i64(call, "offsets"), d_valid=t.u8(call, "valid"), d_result=t.u8(call, "res"), sync=False, **data)
    dev.string_column(d_buf, L, d_fields, so.P_STATUS, d_sel, capacity=rows, bytes_capacity=x.strings.bytes_capacity,
                      **column("string_column", dict(d_bytes=t.u8("string_column", "data"))))
    yield "string_column"
    d_items, d_items_sel = t.records("array_column", "elements"), t.u8("array_column", "esel")
    dev.array_column(*tokens, d_first, d_docs, d_fields, so.P_ITEMS, d_sel, capacity=rows, elements_capacity=x.lists.elements_capacity,
                     d_elements_select=d_items_sel, **numbers, **column("array_column", dict(d_elements=d_items)))
    yield "array_column"
    n_ep = len(so.ELEMENT_POINTERS)
    d_efields, d_esel = t.records("select_elements", "fields")[:n_ep * erows].view(n_ep, erows, 2), t.u8("select_elements", "res")
    dev.select_elements(c.epaths, d_buf, L, *tokens, d_items, d_items_sel, d_fields=d_efields, capacity=erows, d_result=d_esel, sync=False, **numbers)
    yield "select_elements"
    dev.array_elements(*tokens, d_efields[so.E_TAGS], d_esel, capacity=erows, elements_capacity=x.sublists.elements_capacity,
                       d_elements_select=t.u8("array_elements", "esel"), **numbers,
                       **column("array_elements", dict(d_elements=t.records("array_elements", "elements"))))
    yield "array_elements"
    dev.object_entries(*tokens, d_fields[so.P_ATTRS], d_sel, capacity=rows, entries_capacity=x.maps.entries_capacity,
                       d_keys_select=t.u8("object_entries", "ksel"), d_values_select=t.u8("object_entries", "vsel"), **numbers,
                       **column("object_entries", dict(d_keys=t.records("object_entries", "keys"), d_values=t.records("object_entries", "values"))))
    yield "object_entries"
    for compact, call in ((False, "raw_column"), (True, "raw_column_compact")):
        dev.raw_column(d_buf, L, d_idx, n, d_type, d_match, d_end, d_flags, d_fields[so.P_GEO], d_sel, capacity=rows,
                       bytes_capacity=x.raw[compact].bytes_capacity, compact=compact, **column(call, dict(d_bytes=t.u8(call, "data"))))
        yield call
    # (the row count is the column call's own, read where its result lies on the device)
    for source, col, call, want in (("string_column", x.strings, "dictionary_strings", x.dict_strings),
                                    ("raw_column_compact", x.raw[True], "dictionary_raw", x.dict_raw)):
        dev.dictionary(t.i64(source, "offsets"), t.u8(source, "data"), t.u8(source, "valid"), rows=rows, d_n_rows=t.i64(source, "res")[1:2],
                       bytes_len=int(col.res.total_bytes), d_codes=t.i32(call, "codes"), d_dict_offsets=t.i64(call, "dict_offsets"),
                       d_dict_first=t.i32(call, "dict_first"), d_dict_bytes=t.u8(call, "dict_bytes"), dict_capacity=want.dict_capacity,
                       dict_bytes_capacity=want.dict_bytes_capacity, d_result=t.u8(call, "res"), sync=False)
        yield call


def enqueue(c, d_buf, t):
    """The whole chain on the current stream"""
    for _ in chain(c, d_buf, t):
        pass


def raw(t, call, o):
    return t.t[call, o.name].cpu().numpy()


def check(t, where):
    """Every array of every call is the twins', fill and canary included; the dictionaries' max_probe is within its bounds.
    Every call is looked at before the first difference fails the test: the first wrong call is the one that names the cause."""
    x, wrong = t.x, []
    for call, outs in x.calls.items():
        for o in outs:
            mine = raw(t, call, o)
            got, want = o.values(mine), o.values(o.want)
            if o.struct is not None:
                if got != want:
                    wrong.append((call, o.name, dict(zip(o.fields, got)), dict(zip(o.fields, want))))
                if o.struct is _lib.MsjDictionaryResult:
                    longest = int(o.struct.from_buffer_copy(mine.tobytes()).max_probe)
                    if not x.max_probe_holds(call, longest):
                        wrong.append((call, "max_probe", longest))
                continue
            bad = np.nonzero(got != want)[0]
            if bad.size:
                wrong.append((call, o.name, int(bad[0]), got[bad[:4]].tolist(), want[bad[:4]].tolist(), int(bad.size)))
    assert not wrong, (where, x.name, wrong[:12])


def delay_cycles(s, ms):
    """How many cycles of torch.cuda._sleep last `ms` on the stream s, from one unit timed with events"""
    import torch

    unit = SLEEP_UNIT
    while True:   # a unit that lasts 2 ms or more: long against a launch and against the events' resolution
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(s):
            torch.cuda._sleep(unit)   # (the first launch of the kernel is not the one timed)
            e0.record()
            torch.cuda._sleep(unit)
            e1.record()
        s.synchronize()
        unit_ms = e0.elapsed_time(e1)
        if unit_ms >= 2.0 or unit >= 1 << 30:
            break
        unit *= 8
    return int(unit * 1.5 * ms / max(unit_ms, 1e-3)) + unit


def delayed(s, ms):
    """A delay of at least `ms` enqueued on s -> (the event in front of it, for the time it took)"""
    import torch

    cycles = delay_cycles(s, ms)
    start = torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(s):
        start.record()
        while cycles > 0:   # (in pieces that fit any counter)
            torch.cuda._sleep(min(cycles, 1 << 30))
            cycles -= 1 << 30
    return start


def warm(c, t, d_buf):
    """One chain on the default stream, waited for: every workspace of the context has its size -> the host time of the
    enqueue in seconds"""
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    enqueue(c, d_buf, t)
    t_enq = time.perf_counter() - t0
    torch.cuda.synchronize()
    return t_enq


@pytest.mark.gpu
def test_chain_behind_a_late_input(dev):
    """The decoy B is in d_buf and has been through the chain: every tensor and every workspace holds B's consistent
    state.  Then, on a side stream: a delay, a device-to-device copy of A over d_buf, the event `ready`, and the whole chain.
    The enqueue returns while the delay still runs (or the test is inconclusive and fails), and after one synchronisation
    every array is A's.  Work that ran ahead of the stream read B."""
    import torch

    c = Context(dev)
    a, b = so.expected("A"), so.expected("B")
    t = Tensors(dev, a)
    d_buf, d_staging = tvd.upload(dev, b.data), tvd.upload(dev, a.data)
    t_enq = warm(c, t, d_buf)
    s = torch.cuda.Stream(dev.device)
    need_ms = max(MIN_DELAY_MS, JITTER * t_enq * 1e3)
    start, ready = delayed(s, need_ms), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(s):
        d_buf.copy_(d_staging, non_blocking=True)
        ready.record()
        enqueue(c, d_buf, t)
    pending = not ready.query()
    s.synchronize()
    delay_ms = start.elapsed_time(ready)
    numbers = f"the enqueue took {t_enq * 1e3:.2f} ms on the host, the delay {delay_ms:.1f} ms of the {need_ms:.1f} ms it has to last"
    print(numbers)
    assert pending, "inconclusive: the input was there when the enqueue returned -- a host wait in the chain, or the delay too short: " + numbers
    assert delay_ms >= need_ms, numbers
    check(t, "behind a late input")


@pytest.mark.gpu
def test_two_windows_back_to_back(dev):
    """A, C and A again, each into its own tensors, enqueued at once on a side stream behind a delay with no
    synchronisation in between: larger, smaller, larger, so that no workspace grows.  What the host keeps between calls --
    which half of stage 1's workspace is dirty, whose aggregates the token workspace holds -- does not depend on a call
    having completed."""
    import torch

    c = Context(dev)
    a, x = so.expected("A"), so.expected("C")
    sets = [Tensors(dev, a), Tensors(dev, x), Tensors(dev, a)]
    bufs = {a.name: tvd.upload(dev, a.data), x.name: tvd.upload(dev, x.data)}
    warm(c, sets[0], bufs["A"])
    s = torch.cuda.Stream(dev.device)
    delayed(s, MIN_DELAY_MS)
    with torch.cuda.stream(s):
        for t in sets:
            enqueue(c, bufs[t.x.name], t)
    s.synchronize()
    for k, t in enumerate(sets):
        check(t, ("back to back", k))


def identical(sets, where):
    """The same bytes in every set of tensors (of one window): all that check() compares, bit for bit"""
    first = sets[0]
    for t in sets[1:]:
        for call, outs in first.x.calls.items():
            for o in outs:
                mine, theirs = o.values(raw(first, call, o)), o.values(raw(t, call, o))
                assert np.array_equal(mine, theirs), (where, call, o.name)


@pytest.mark.gpu
def test_dirty_context_equals_fresh():
    """C on a fresh context, on one that has just run A, and on one that has just run A with the small limits of
    msj_debug_set_span_limits (long stretches read from memory, the list of long strings of 3 entries overflowed by A's five bodies over 1 024 bytes,
    the lists emptied again): the same bytes, and the twins'.  A context's workspaces grow and are never cleared; a call's
    outputs are a function of its inputs all the same."""
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    a, x = so.expected("A"), so.expected("C")
    sets, contexts = [], []
    try:
        for limits in (None, (0xFFFFFFFF, 0xFFFFFFFF), SMALL_LIMITS):
            c = Context()
            contexts.append(c)
            if limits is not None:
                c.dev.lib.msj_debug_set_span_limits(c.dev.ctx, *limits)
                before = Tensors(c.dev, a)
                enqueue(c, tvd.upload(c.dev, a.data), before)
                c.dev.lib.msj_debug_set_span_limits(c.dev.ctx, 0xFFFFFFFF, 0xFFFFFFFF)
            t = Tensors(c.dev, x)
            enqueue(c, tvd.upload(c.dev, x.data), t)
            torch.cuda.synchronize()
            if limits is not None:
                check(before, ("A in front", limits))
            check(t, ("C behind", limits))
            sets.append(t)
        identical(sets, "fresh, dirty, dirty with small limits")
    finally:
        for c in contexts:
            c.close()


@pytest.mark.gpu
def test_two_contexts_two_streams():
    """Two contexts on two side streams, A on one and the decoy B on the other, the calls behind stage2_prep enqueued in
    turns with nothing waited for: device state that the process holds once would be shared by the two."""
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    contexts = [Context(), Context()]
    try:
        windows = [so.expected("A"), so.expected("B")]
        sets = [Tensors(c.dev, x) for c, x in zip(contexts, windows)]
        bufs = [tvd.upload(c.dev, x.data) for c, x in zip(contexts, windows)]
        for c, t, d_buf in zip(contexts, sets, bufs):
            warm(c, t, d_buf)
        streams = [torch.cuda.Stream(c.dev.device) for c in contexts]
        chains = [chain(c, d_buf, t) for c, t, d_buf in zip(contexts, sets, bufs)]
        for s, calls in zip(streams, chains):   # stage 1 and the prep call of each first, and waited for
            with torch.cuda.stream(s):
                for call in calls:
                    if call == "stage2_prep":
                        break
        torch.cuda.synchronize()
        live = list(zip(streams, chains))
        while live:
            for s, calls in list(live):
                with torch.cuda.stream(s):
                    if next(calls, None) is None:
                        live.remove((s, calls))
        for s in streams:
            s.synchronize()
        for t in sets:
            check(t, "two contexts")
    finally:
        for c in contexts:
            c.close()


@pytest.mark.gpu
def test_document_stream_on_a_side_stream(dev):
    """DocumentStream(select=..., parse=True, validate=True) over A + C entirely under a side stream, the upload included:
    documents(), values, strings, elements, entries, raw and categories are json.loads' and tdc.definition's, as the
    end-to-end tests of the calls check them on the default stream.  (A's longest document has more than 16 KiB: the windows
    are the fewest multiples of 8 KiB that hold it.)"""
    import torch
    from mojo_simdjson_amd.document_stream import DocumentStream

    a, c = so.expected("A"), so.expected("C")
    lines, data = a.lines + c.lines, a.data + c.data
    docs = [None if code else json.loads(text) for code, text in zip(a.codes + c.codes, lines)]
    window = WINDOW * -(-(max(len(text) for text in lines) + 17) // WINDOW)
    has = lambda d, key, kind: d is not None and isinstance(d.get(key), kind)

    def rows_of(column, n):
        offsets, out, valid = column
        assert offsets.is_cuda and out.is_cuda and offsets.shape == (n + 1,) and valid.shape == (n,)
        off, text, ok = offsets.cpu().tolist(), out.cpu().numpy().tobytes(), valid.cpu().tolist()
        return [text[off[k]:off[k + 1]] if ok[k] else None for k in range(n)]

    s = torch.cuda.Stream(dev.device)
    seen = windows = 0
    with torch.cuda.stream(s):
        d_buf = tvd.upload(dev, data)
        for win in DocumentStream(dev, d_buf, len(data), window=window, select=so.POINTERS, parse=True, validate=True):
            assert torch.cuda.current_stream(dev.device) == s
            D = win.n_documents
            mine = docs[seen:seen + D]
            where = (windows, seen)
            assert [d.to_python() if d is not None else None for d in win.documents()] == mine, where
            for p in so.POINTERS:
                assert win.values(p) == [None if d is None else d if p == "" else d.get(p[1:]) for d in mine], (where, p)
            status = [d["status"].encode() if has(d, "status", str) else None for d in mine]
            assert rows_of(win.strings("/status"), D) == status, where
            assert win.elements("/tags").to_python() == [d["tags"] if has(d, "tags", list) else None for d in mine], where
            assert win.entries("/attrs").to_python() == [d["attrs"] if has(d, "attrs", dict) else None for d in mine], where
            geo = [json.dumps(d["geo"], separators=(",", ":")).encode() if has(d, "geo", dict) else None for d in mine]
            assert rows_of(win.raw("/geo", compact=True), D) == geo, where
            assert [r and json.loads(r) for r in rows_of(win.raw("/geo"), D)] == [g and json.loads(g) for g in geo], where
            cats = win.categories("/status")
            codes, distinct, first = tdc.definition(status)
            got_values, got_codes = cats.to_python()
            assert got_codes == codes and got_values == [v.decode() for v in distinct] and cats.first.cpu().tolist() == first, where
            assert cats.counts().cpu().tolist() == [codes.count(k) for k in range(len(distinct))], where
            seen += D
            windows += 1
    s.synchronize()
    assert windows >= 8 and seen == len(docs)
