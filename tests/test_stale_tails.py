"""Every device call behind stage 1 on arrays that hold a larger window's leftovers (tests/stale_tails.py: the windows, the
three stale states, what a call writes).

DocumentStream allocates its arrays once with torch.empty and never clears them, so a short window that follows a long one
runs with the long one's tokens, flags, partners, records and rows behind its own counts.  The other tests of these calls
put one constant byte (or whatever the allocator holds) there.  Here one set of tensors serves every window: each array has
the size the largest window needs plus SLACK elements, a copy in stream order puts a stale state into ALL of them, and the
chain of tests/test_stream_order.py runs over it with the window's own n, D and capacities and without a refill.  Every
output array is then compared over the WHOLE tensor, slack included: the twin's bytes where the call writes, the stale
state's, untouched, everywhere else.  A kernel whose last unit reads or writes behind its count shows as a wrong array;
every stale value is in bounds of the test's allocations, so it cannot show as a fault.

Arrays that are not described as "the twin's bytes over a counted prefix, the state's behind it":
    tape_documents / sbuf  a document with a verdict code keeps its slot of the string buffer, with unspecified contents
                           (include/msj_stage1.h); the twin and the kernel leave it alone, so the slot counts as untouched
                           and has to hold the stale state (st.string_slots)
    shard / idx            stage 1 leaves a trailer behind its n indices that no caller may read (so.Out.upto): the first n
                           indices are compared, nothing behind them
    the result structs     compared field by field as tests/test_stream_order.py does (n_slow and max_probe have no twin)
"""
import time

import numpy as np
import pytest

from mojo_simdjson_amd import _lib
from tests import stale_tails as st
from tests import stream_order as so
from tests import test_stream_order as tso
from tests import test_tape_documents as ttd
from tests import test_validate_documents as tvd

PARENT_CORPUS_SECONDS = 12.2   # tests/test_stream_order.py::test_corpus_on_cpu at the parent commit, where the windows here took 2.4 s
LIMITS = (None, tso.SMALL_LIMITS)


def listed(wrong, *where):
    """The first differences, one per line (an assertion's message is cut short otherwise)"""
    return "\n".join(repr(w) for w in list(where) + wrong[:12])


# ---- the corpus, on the CPU -----------------------------------------------------------------------------------------------------

def test_corpus_on_cpu():
    """The windows have the token counts and document counts that leave every unit partly filled, every stale value that
    could serve as an index is in bounds of the allocations, and what `written` says a call writes is exactly what the
    window's counts say: no position accepts two values."""
    t0 = time.perf_counter()
    windows = [st.expected(r) for r in st.REMAINDERS]
    seconds = time.perf_counter() - t0
    print(f"the {len(windows)} windows took {seconds:.1f} s to build (A and B, cached, included); the three windows of "
          f"tests/test_stream_order.py::test_corpus_on_cpu took {PARENT_CORPUS_SECONDS} s with their checks")
    a = so.expected("A")
    for r, x in zip(st.REMAINDERS, windows):
        print(f"window {x.name}: n = {x.n} = {x.n // st.PHASE} x {st.PHASE} + {x.n % st.PHASE}, D = {x.D} (mod 256: {x.D % 256}, mod 64: {x.D % 64}), "
              f"{x.ncap} numbers, E = {x.E}, {int(x.maps.res.n_entries)} entries, {x.length} bytes")
        assert x.n % st.PHASE == r and x.D == st.DOCUMENTS[r] and x.lines[:-1] == a.lines[:x.D - 1]
        assert x.n <= a.n and x.length <= a.length and x.ncap <= a.ncap
        # the codes: 0 but for the document that is invalid on purpose; it and an escaped body over 1 024 bytes are in every window
        assert x.vres.code == 0 and x.tape.res.code == 0 and x.sel.res.code == 0
        assert x.D - 1 > max(so.INVALID, so.ESCAPED_1K[0]) and [k for k, code in enumerate(x.codes) if code] == [so.INVALID]
        w = x.w
        size = w.end.astype(np.int64) - w.idx.astype(np.int64)
        assert int(((w.typ == ord('"')) & ((w.flags & 2) != 0) & (size - 1 > 1024)).sum()) >= 1
    assert {x.D % 256 for x in windows} >= {0, 1, 255} and {x.D % 64 for x in windows} >= {1, 63}
    assert {x.n % 2048 for x in windows} >= {0, 1, 2047} and {x.n % 8 for x in windows} >= {0, 1, 7} and {x.n % 4 for x in windows} == {0, 1, 2, 3}
    assert max(x.n for x in windows) <= 40000 and st.poison_tokens() == min(x.n for x in windows) > 2048

    # the tensors hold every window with SLACK elements to spare; every canary is a whole number of elements
    sizes = st.sizes()
    for x in windows + [a, so.expected("B")]:
        ext = st.extents(x)
        for call, o in st.arrays(x):
            width = st.WIDTH[o.name]
            assert o.want.size % width == 0 or o.name in st.TEXT + st.BYTES, (x.name, call, o.name)
            assert o.want.size + st.SLACK * width <= sizes[call, o.name], (x.name, call, o.name)
            # the mask from the twin's bytes is the counted extent: nothing all-fill inside, all fill behind
            counted = np.zeros(o.want.size, dtype=bool)
            for lo, hi in ext[call, o.name]:
                assert 0 <= lo <= hi and hi * width <= o.want.size
                counted[lo * width:hi * width] = True
            assert np.array_equal(st.written(x, call, o, ext), counted), (x.name, call, o.name)
            assert (o.want[~counted] == o.fill).all(), (x.name, call, o.name)
            if o.upto is not None:
                assert o.upto == int(counted.sum())
        assert len(st.window_bytes(x)) == st.buffer_length()

    # the stale states: in bounds, and behind every window's counts something other than the array's fill
    for state in st.STATES:
        assert st.out_of_bounds(state) == [], state
    for x in windows:
        ext = st.extents(x)
        for state in st.STATES:
            before, after = st.stale(state), st.full_want(x, state)
            for call, o in st.arrays(x):
                full, upto = after[call, o.name]
                assert full.size == sizes[call, o.name] and upto <= full.size
                untouched = np.ones(full.size, dtype=bool)
                untouched[:o.want.size] = ~st.written(x, call, o, ext)
                assert np.array_equal(full[untouched], before[call, o.name][untouched]) and (full[untouched] != o.fill).any(), (x.name, state, call, o.name)
    # the poison's types behind a stream: a closing bracket among any two neighbours (the apply_depth pin below)
    assert all(set((st.TYPES * 2)[k:k + 2]) & set(b"]}") for k in range(len(st.TYPES)))

    # the calls outside the chain: the oracle's arrays are the chain's, the records behind D look live
    for r in (1, 2049, 4095):
        x, tc = st.expected(r), st.token_calls(r)
        assert np.array_equal(tc.type, x.w.typ) and np.array_equal(tc.depth, x.w.depth) and np.array_equal(tc.end, x.w.end)
        assert tc.result == (x.tokens.n, x.tokens.final_depth, x.tokens.min_depth, x.tokens.max_depth, x.tokens.reserved)
        assert tc.result[1:3] == (0, 0)   # the stream ends at depth 0 and never goes below: one stale closing bracket shows
        for state in st.STATES:
            rc = st.RowCalls(x, state)
            records = st.full_want(x, state)["select_documents", "fields"][0].view(st.FIELD_DTYPE)
            assert (records["code"][so.P_STATUS * x.rows + x.D:(so.P_STATUS + 1) * x.rows] == 0).all(), "the records behind D look live"
            assert (rc.filtered.keep[x.D:] == 0x77).all()


# ---- on the device ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def dev():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mojo_simdjson_amd.device import Stage1Device

    d = Stage1Device(0)
    yield d
    d.close()


class Tensors(tso.Tensors):
    """One set of tensors for every window: each of st.sizes() bytes, and beside each the three stale states"""

    def __init__(self, dev):
        import torch

        self.x, self.t = None, {}
        for key, size in st.sizes().items():
            self.t[key] = torch.zeros(size, dtype=torch.uint8, device=dev.device)
        self.states = {state: {key: ttd.to_device(dev, full) for key, full in st.stale(state).items()} for state in st.STATES}
        self.zero = dev.new_carry()

    def load(self, state):
        """The stale state into every array, on the current stream"""
        for key, d in self.t.items():
            d.copy_(self.states[state][key], non_blocking=True)


class Rig:
    """The context with its paths, the tensors, the window's buffer"""

    def __init__(self, dev):
        import torch

        self.c, self.dev = tso.Context(dev), dev
        self.t = Tensors(dev)
        self.d_buf = torch.zeros(st.buffer_length(), dtype=torch.uint8, device=dev.device)

    def run(self, x, state):
        """The window's chain over the stale state, enqueued with sync=False and waited for once -> {(call, array): bytes}"""
        import torch

        t = self.t
        t.x = x
        self.d_buf.copy_(tvd.upload(self.dev, st.window_bytes(x)), non_blocking=True)
        t.load(state)
        for _ in tso.chain(self.c, self.d_buf, t, refill=False):
            pass
        torch.cuda.synchronize()
        return {key: d.cpu().numpy() for key, d in t.t.items()}


@pytest.fixture(scope="module")
def rig(dev):
    r = Rig(dev)
    # all of A first: every workspace of the context has its largest size, and holds a longer window's state
    got = r.run(so.expected("A"), "continuation")
    wrong = differences(so.expected("A"), "continuation", got)
    assert not wrong, listed(wrong, "A over its own state")
    return r


def differences(x, state, got):
    """Every array of every call over the whole tensor, every result struct field by field -> what differs.  Every call is
    looked at: the first wrong call is the one that names the cause."""
    wrong, want, ext = [], st.full_want(x, state), st.extents(x)
    for call, outs in x.calls.items():
        for o in outs:
            mine = got[call, o.name]
            if o.struct is not None:
                a, b = o.values(mine), o.values(o.want)
                if a != b:
                    wrong.append((call, o.name, dict(zip(o.fields, a)), dict(zip(o.fields, b))))
                if o.struct is _lib.MsjDictionaryResult:
                    longest = int(o.struct.from_buffer_copy(mine.tobytes()).max_probe)
                    if not x.max_probe_holds(call, longest):
                        wrong.append((call, "max_probe", longest))
                continue
            full, upto = want[call, o.name]
            assert mine.size == full.size
            bad = np.nonzero(mine[:upto] != full[:upto])[0]
            if bad.size:
                width = st.WIDTH[o.name]
                inside = any(lo * width <= int(bad[0]) < hi * width for lo, hi in ext[call, o.name])
                wrong.append((call, o.name, "element %d, %s" % (int(bad[0]) // width, "written by the call" if inside else "BEHIND what the call writes"),
                              mine[bad[:4]].tolist(), full[bad[:4]].tolist(), int(bad.size)))
    return wrong


def compared(x, got):
    """What the three stale runs of a window have to agree in, bit for bit: the bytes each call writes and the structs' fields"""
    ext, out = st.extents(x), {}
    for call, outs in x.calls.items():
        for o in outs:
            mine = got[call, o.name]
            out[call, o.name] = o.values(mine) if o.struct is not None else mine[:o.want.size][st.written(x, call, o, ext)]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("r", st.REMAINDERS)
def test_chain_over_stale_arrays(rig, r):
    """The whole chain over window r on the decoy's, the continuation's and the poison's leftovers: every array over the
    whole tensor is the twin's where the call writes and the state's elsewhere, and the three runs agree bit for bit in
    everything a call writes."""
    x = st.expected(r)
    runs, wrong = {}, []
    for state in st.STATES:
        got = rig.run(x, state)
        wrong += [(state,) + w for w in differences(x, state, got)]
        runs[state] = compared(x, got)
    assert not wrong, listed(wrong, (x.name, x.n, x.D))
    first = runs[st.STATES[0]]
    for state in st.STATES[1:]:
        for key, mine in first.items():
            theirs = runs[state][key]
            assert mine == theirs if isinstance(mine, tuple) else np.array_equal(mine, theirs), (x.name, state, key)


@pytest.mark.gpu
@pytest.mark.parametrize("r", st.REMAINDERS)
def test_row_calls_over_stale_records(rig, r):
    """filter_rows, take_rows and cast_strings over the records a stale run's select_documents leaves, capacity = rows: the
    ROOM records behind the D of every path are stale and look live.  Whole arrays against the twins, fill and canary
    included, as tests/test_filter_rows_stream_order.py and tests/test_cast_strings_stream_order.py compare them."""
    import torch

    dev, x = rig.dev, st.expected(r)
    n_paths, rows, wrong = len(so.POINTERS), x.rows, []
    for state in st.STATES:
        rig.run(x, state)
        want = st.RowCalls(x, state)
        arrays = want.arrays()
        out = {name: ttd.to_device(dev, np.full(w.size, 0x77, dtype=np.uint8)) for name, w in arrays.items()}
        predicates = dev.compile_predicates(want.device_specs, any=False)
        d_fields = rig.t.records("select_documents", "fields")[:n_paths * rows].view(n_paths, rows, 2)
        d_sel = rig.t.u8("select_documents", "res")
        records = lambda name, shape: out[name].view(torch.int64)[:2 * int(np.prod(shape))].view(*shape, 2)
        dev.filter_rows(predicates, rig.d_buf, x.length, d_fields, d_sel, capacity=rows, d_keep=out["keep"], d_kept=out["kept"].view(torch.int32),
                        d_result=out["res"], d_kept_select=out["ksel"], sync=False)
        dev.take_rows(out["kept"].view(torch.int32), out["ksel"], d_fields, d_sel, d_out=records("out", (n_paths, rows)), out_capacity=rows,
                      d_result=out["tres"], d_out_select=out["osel"], sync=False)
        for kind in want.casts:
            dev.cast_strings(rig.d_buf, x.length, d_fields[so.P_STATUS], d_sel, kind, "ms", False, capacity=rows, d_out=records(f"cast_{kind}", (rows,)),
                             d_result=out[f"cres_{kind}"], d_out_select=out[f"csel_{kind}"], sync=False)
        torch.cuda.synchronize()
        predicates.close()
        for name, w in arrays.items():
            got = out[name].cpu().numpy()
            bad = np.nonzero(got != w)[0]
            if bad.size:
                wrong.append((state, name, int(bad[0]), got[bad[:4]].tolist(), w[bad[:4]].tolist(), int(bad.size)))
    assert not wrong, listed(wrong, (x.name, x.D))


# ---- the calls outside the chain ------------------------------------------------------------------------------------------------

class Outside:
    """The caller's arrays of the token calls for one window in one stale state, on the device"""

    def __init__(self, dev, tc, state):
        self.dev, self.tc, self.state = dev, tc, state
        self.d_buf = tvd.upload(dev, st.window_bytes(tc.x))
        self.d_idx = ttd.to_device(dev, tc.inputs(state, "idx")).view(_torch().int32)
        self.d = {}

    def array(self, name, dtype):
        """A fresh copy of the stale array `name`"""
        self.d[name] = ttd.to_device(self.dev, self.tc.before(self.state, name)).view(dtype)
        return self.d[name]

    def result(self):
        self.d_res = _torch().zeros(24, dtype=_torch().uint8, device=self.dev.device)
        return self.d_res

    def wrong(self, where, names, fields=4):
        """The arrays `names` over the whole tensors -- the oracle's over [0, n), untouched behind -- and the first `fields`
        fields of the result (0: the call has none)"""
        out = []
        res = _lib.MsjTokensResult.from_buffer_copy(self.d_res.cpu().numpy().tobytes()) if fields else None
        mine = (res.n, res.final_depth, res.min_depth, res.max_depth, res.reserved)[:fields] if fields else ()
        if mine != self.tc.result[:fields]:
            out.append((where, self.state, "the result (n, final, min, max depth, opening brackets)", mine, self.tc.result[:fields]))
        for name in names:
            got, want = self.d[name].view(_torch().uint8).cpu().numpy(), self.tc.after(self.state, name)
            bad = np.nonzero(got != want)[0]
            if bad.size:
                width = 8 if name == "pairs" else st.WIDTH[name]
                at, n_written = int(bad[0]) // width, self.tc.want(name).size // width
                out.append((where, self.state, name, "element %d, %s" % (at, "in [0, n)" if at < n_written else "BEHIND n"),
                            got[bad[:4]].tolist(), want[bad[:4]].tolist(), int(bad.size)))
        return out


def _torch():
    import torch

    return torch


def outside_cases(dev, r):
    """(where, Outside) for the decoy and the poison, with the default span limits and with SMALL_LIMITS"""
    tc = st.token_calls(r)
    for limits in LIMITS:
        dev.lib.msj_debug_set_span_limits(dev.ctx, *(limits or (0xFFFFFFFF, 0xFFFFFFFF)))
        try:
            for state in st.OUTSIDE_STATES:
                yield f"{tc.x.name}, limits {limits}", Outside(dev, tc, state)
        finally:
            dev.lib.msj_debug_set_span_limits(dev.ctx, 0xFFFFFFFF, 0xFFFFFFFF)


@pytest.mark.gpu
@pytest.mark.parametrize("match", [True, False], ids=["match", "depth"])
@pytest.mark.parametrize("r", st.REMAINDERS)
def test_tokens_on_stale_arrays(dev, r, match):
    """dev.tokens into arrays that hold another stream behind n, against helpers.oracle_tokens / oracle_match, the
    result's final / minimum / maximum depth included, and untouched behind n.

    With match=True and n mod 2 048 = 1 (windows S1 and S2049) this is the small pin of the hipcc 7.2 miscompile that
    apply_depth met (csrc/tokens_kernel.hip, DESIGN.md "A hipcc 7.2 miscompile met on the way"): the stream's last block ran
    with nrem = 2 048 and folded the stale type bytes behind the stream's end into the minimum depth.  Here those bytes
    are the decoy's tokens or the poison's closing brackets, and the stream ends at depth 0 with minimum 0.  With that
    failure put back by hand (nrem = kBlock whatever n, tried once on a copy of the tree) both windows fail here: the
    decoy gives the result (20481, 0, -2, 5) for S1's (20481, 0, 0, 5) and a minimum of -1 for S2049, and the partners
    behind n are overwritten in either state."""
    torch, wrong = _torch(), []
    for where, o in outside_cases(dev, r):
        arrays = dict(d_type=o.array("type", torch.uint8), d_depth=o.array("depth", torch.int32))
        if match:
            arrays["d_match"] = o.array("match", torch.int32)
        dev.tokens(o.d_buf, o.tc.x.length, o.d_idx, o.tc.n, match=match, d_result=o.result(), sync=False, **arrays)
        torch.cuda.synchronize()
        wrong += o.wrong(where, ["type", "depth"] + ["match"] * match)
    assert not wrong, listed(wrong)


@pytest.mark.gpu
@pytest.mark.parametrize("r", st.REMAINDERS)
def test_token_spans_on_stale_arrays(dev, r):
    """msj_token_spans_device (dev.token_spans with the caller's arrays) against oracle/tokens_oracle.c, untouched behind n"""
    from mojo_simdjson_amd.device import _ptr

    torch, wrong = _torch(), []
    for where, o in outside_cases(dev, r):
        d_end, d_flags = o.array("end", torch.int32), o.array("flags", torch.uint8)
        rc = dev.lib.msj_token_spans_device(dev.ctx, _ptr(o.d_buf), o.tc.x.length, _ptr(o.d_idx), o.tc.n, _ptr(d_end), _ptr(d_flags), dev._stream())
        assert rc == 0
        torch.cuda.synchronize()
        wrong += o.wrong(where, ["end", "flags"], fields=0)
    assert not wrong, listed(wrong)


@pytest.mark.gpu
@pytest.mark.parametrize("spans", [True, False], ids=["prep", "tokens"])
@pytest.mark.parametrize("r", st.REMAINDERS)
def test_pairs_on_stale_arrays(dev, r, spans):
    """msj_stage2_prep_pairs_device / msj_tokens_pairs_device (dev.stage2_prep_pairs with the caller's arrays) against
    oracle/tokens_oracle.c: a record per opening bracket, the records behind them and everything behind n untouched"""
    from mojo_simdjson_amd.device import _ptr

    torch, wrong = _torch(), []
    for where, o in outside_cases(dev, r):
        d_type, d_depth, d_pairs = o.array("type", torch.uint8), o.array("depth", torch.int32), o.array("pairs", torch.int32)
        common = (dev.ctx, _ptr(o.d_buf), o.tc.x.length, _ptr(o.d_idx), o.tc.n, _ptr(d_type), _ptr(d_depth), _ptr(d_pairs))
        if spans:
            d_end, d_flags = o.array("end", torch.int32), o.array("flags", torch.uint8)
            rc = dev.lib.msj_stage2_prep_pairs_device(*common, _ptr(d_end), _ptr(d_flags), _ptr(o.result()), None, dev._stream())
        else:
            rc = dev.lib.msj_tokens_pairs_device(*common, _ptr(o.result()), None, dev._stream())
        assert rc == 0
        torch.cuda.synchronize()
        wrong += o.wrong(where, ["type", "depth", "pairs"] + ["end", "flags"] * spans, fields=5)
    assert not wrong, listed(wrong)


@pytest.mark.gpu
@pytest.mark.parametrize("match", [True, False], ids=["match", "depth"])
@pytest.mark.parametrize("r", st.REMAINDERS)
def test_depth_from_types_on_stale_arrays(dev, r, match):
    """dev.depth_from_types: d_type is an input -- the window's types, the stale tail behind them -- against
    helpers.oracle_tokens / oracle_match, the result's depths included, d_type itself and everything behind n untouched"""
    torch, wrong = _torch(), []
    for where, o in outside_cases(dev, r):
        o.d["type"] = ttd.to_device(dev, o.tc.inputs(o.state, "type"))
        arrays = dict(d_depth=o.array("depth", torch.int32))
        if match:
            arrays["d_match"] = o.array("match", torch.int32)
        dev.depth_from_types(o.d["type"], o.tc.n, match=match, d_result=o.result(), **arrays)
        torch.cuda.synchronize()
        wrong += o.wrong(where, ["type", "depth"] + ["match"] * match)
    assert not wrong, listed(wrong)
