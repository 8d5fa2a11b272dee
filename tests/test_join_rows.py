"""The equi-join of two code columns on the device (msj_join_rows_device, csrc/join_rows_kernel.hip), through the C ABI.

Expected values come from the host twin of the same arithmetic (tests/join_rows_math_host.cpp), which
tests/test_join_rows_math.py holds against the definition written in Python, and from that definition itself in its numpy
form (``np_join``: a stable sort and searchsorted; it shares nothing with the kernels).  Device output is compared with both
over WHOLE tensors: d_left_rows, d_right_rows and d_offsets start from the fill 0xA5 with a canary behind the room, so a store
at or past M, pairs_capacity or d_offsets[L] shows; the 64-byte result and both select results byte for byte.

The kernel's constants (csrc/join_rows_kernel.hip) as the shapes use them: kRows = 256 lanes, kTile = 1 024 rows, keys or
pairs per block, 8-bit digits (the borders of G are 256 / 65 536 / 2^24: one to four passes; G = 1 takes one pass as well,
the pass that leaves out the rows without a key), kStage = 1 025 offsets staged per emit block.
"""
import ctypes

import numpy as np
import pytest

from mojo_simdjson_amd import _lib
from tests import test_join_rows_math as tjm

pytestmark = pytest.mark.gpu

B = 256            # kRows
T = 1024           # kTile
CANARY = 16        # entries behind every output's room
KINDS = tjm.KINDS
INNER, LEFT, SEMI, ANTI = KINDS
FILL, FILL32, FILL64, NO_ROW = tjm.FILL, tjm.FILL32, tjm.FILL64, tjm.NO_ROW
MSJ_CAPACITY = 1
POISON = 0x5A5A5A5A


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
def jtw():
    return tjm.load_twin()


def to_dev(dev, a, dtype):
    import torch

    a = np.ascontiguousarray(a)
    if a.size == 0:
        return torch.zeros((1,), dtype=dtype, device=dev.device)
    return torch.from_numpy(a.view({4: np.int32, 8: np.int64}[a.itemsize]).copy()).to(dev.device)


class Held:
    """A call's tensors on the device: the keys, the outputs with their canaries, the results; the outputs filled with FILL"""

    def __init__(self, dev, lk, rk, room):
        import torch

        self.dev, self.room, self.left_rows, self.right_rows = dev, room, len(lk), len(rk)
        self.d_lk, self.d_rk = to_dev(dev, lk, torch.int32), to_dev(dev, rk, torch.int32)
        self.t_left = torch.empty((room + CANARY,), dtype=torch.int32, device=dev.device)
        self.t_right = torch.empty((room + CANARY,), dtype=torch.int32, device=dev.device)
        self.t_off = torch.empty((len(lk) + 1 + CANARY,), dtype=torch.int64, device=dev.device)
        self.t_res = torch.empty((64,), dtype=torch.uint8, device=dev.device)
        self.t_lsel = torch.empty((48,), dtype=torch.uint8, device=dev.device)
        self.t_rsel = torch.empty((48,), dtype=torch.uint8, device=dev.device)
        self.refill()

    def refill(self):
        self.t_left.fill_(FILL32 - 2**32), self.t_right.fill_(FILL32 - 2**32), self.t_off.fill_(FILL64 - 2**64)
        self.t_res.fill_(FILL), self.t_lsel.fill_(FILL), self.t_rsel.fill_(FILL)

    def call(self, G, kind, counts=None, keys_capacity=None, pairs_capacity=None, want_right=True, want_offsets=True, want_selects=True,
             host_G=None):
        """One call -> everything it left, on the host.  counts: (L, R, G) given on the device only"""
        import torch

        dev = self.dev
        d_counts = None if counts is None else torch.tensor([-1 if c is None else c for c in counts], dtype=torch.int64, device=dev.device)
        ptr = lambda i: None if counts is None or counts[i] is None else d_counts.data_ptr() + 8 * i
        room = self.room if pairs_capacity is None else pairs_capacity
        rc = dev.lib.msj_join_rows_device(dev.ctx, self.d_lk.data_ptr() if self.left_rows else None, self.left_rows, ptr(0),
                                          self.d_rk.data_ptr() if self.right_rows else None, self.right_rows, ptr(1),
                                          G if host_G is None else host_G, ptr(2), G if keys_capacity is None else keys_capacity, kind,
                                          self.t_left.data_ptr() if room else None, self.t_right.data_ptr() if room and want_right else None, room,
                                          self.t_off.data_ptr() if want_offsets else None, self.t_res.data_ptr(),
                                          self.t_lsel.data_ptr() if want_selects else None, self.t_rsel.data_ptr() if want_selects else None,
                                          dev._stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        return (self.t_left.cpu().numpy().view(np.uint32), self.t_right.cpu().numpy().view(np.uint32), self.t_off.cpu().numpy().view(np.uint64),
                self.t_res.cpu().numpy(), self.t_lsel.cpu().numpy(), self.t_rsel.cpu().numpy())


def with_fill(a, room, fill, dtype):
    out = np.full(room + CANARY, fill, dtype=dtype)
    if a is not None:
        out[:len(a)] = a
    return out


def run_join(dev, jtw, lk, rk, G, kind, L=None, R=None, G_dev=None, keys_capacity=None, pairs_capacity=None, where=None, held=None,
             want_right=True, want_offsets=True, want_selects=True, runs=1):
    """The device against the twin and the numpy definition over every output's whole tensor -> (the twin's Joined, Held)"""
    lk, rk = np.ascontiguousarray(lk, dtype=np.int32), np.ascontiguousarray(rk, dtype=np.int32)
    eff_L, eff_R, eff_G = (len(lk) if L is None else L), (len(rk) if R is None else R), (G if G_dev is None else G_dev)
    stop = eff_L > len(lk) or eff_R > len(rk) or eff_G > (G if keys_capacity is None else keys_capacity)
    definition = None if stop else tjm.np_join(lk, rk, eff_L, eff_R, eff_G, kind)
    if pairs_capacity is None:
        pairs_capacity = 0 if stop else definition[3][0]
    want = tjm.twin_join(jtw, lk, rk, G, kind, L=L, R=R, G_dev=G_dev, keys_capacity=keys_capacity, pairs_capacity=pairs_capacity)
    assert want.rc == 0
    if definition is not None:          # the twin is the definition (its own CPU tests hold the small cases)
        M = definition[3][0]
        assert want.counters() == definition[3], where
        assert np.array_equal(want.offsets[:eff_L + 1], definition[2]), where
        if M <= pairs_capacity:
            assert np.array_equal(want.left[:M], definition[0]) and np.array_equal(want.right[:M], definition[1]), where
    held = held or Held(dev, lk, rk, pairs_capacity)
    want_res = np.frombuffer(bytes(want.res), dtype=np.uint8)
    want_sel = np.frombuffer(bytes(want.lsel), dtype=np.uint8)
    assert bytes(want.lsel) == bytes(want.rsel)
    exp_left = with_fill(want.left, held.room, FILL32, np.uint32)
    exp_right = with_fill(want.right if want_right else None, held.room, FILL32, np.uint32)
    exp_off = with_fill(want.offsets if want_offsets else None, len(lk) + 1, FILL64, np.uint64)
    counts = None if L is None and R is None and G_dev is None else (L, R, G_dev)
    first = None
    for run in range(runs):
        held.refill()
        got = held.call(G, kind, counts, keys_capacity, pairs_capacity, want_right, want_offsets, want_selects)
        left, right, off, res, lsel, rsel = got
        r = _lib.MsjJoinRowsResult.from_buffer_copy(res.tobytes())
        assert np.array_equal(res, want_res), (where, [(n, getattr(r, n), getattr(want.res, n)) for n, _ in r._fields_])
        for name, a, b in (("left rows", left, exp_left), ("right rows", right, exp_right), ("offsets", off, exp_off)):
            bad = np.nonzero(a != b)[0]
            assert bad.size == 0, (where, name, "entry", int(bad[0]), int(a[bad[0]]), int(b[bad[0]]), int(bad.size), int(want.res.n_pairs))
        for s in (lsel, rsel):
            assert np.array_equal(s, want_sel if want_selects else np.full(48, FILL, dtype=np.uint8)), (where, "select result")
        if first is None:
            first = got
        else:
            assert all(np.array_equal(a, b) for a, b in zip(first, got)), (where, "two runs differ")
    return want, held


def keys_with_nulls(rng, n, G, span=None, nulls=0.1):
    k = rng.integers(0, span or G, n, dtype=np.int64)
    bad = rng.random(n) < nulls
    k[bad] = rng.choice(np.array([-1, -2, G, G + 5, 2**31 - 1, -2**31]), int(bad.sum()))
    return k.astype(np.int32)


@pytest.mark.parametrize("kind", KINDS)
def test_kinds_with_nulls_on_both_sides(dev, jtw, kind):
    rng = np.random.default_rng(kind)
    lk, rk = keys_with_nulls(rng, 3000, 700), keys_with_nulls(rng, 2500, 700)
    want, held = run_join(dev, jtw, lk, rk, 700, kind, runs=2)
    assert want.res.n_left_null and want.res.n_right_null and want.res.n_pairs
    run_join(dev, jtw, lk, rk, 700, kind, held=held, pairs_capacity=held.room, want_right=False, want_offsets=False, want_selects=False, where="no optional output")


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513, T - 1, T, T + 1, 2 * T + 1])
def test_row_counts_around_the_waves_and_the_tile(dev, jtw, n):
    """L and R on both sides of a wave, L and R mod 256 in {0, 1, 255}, and one row past a radix tile (kTile = 1 024)"""
    rng = np.random.default_rng(n)
    for kind in KINDS:
        run_join(dev, jtw, keys_with_nulls(rng, n, 300), keys_with_nulls(rng, 777, 300), 300, kind, where=("L", n, kind))
        run_join(dev, jtw, keys_with_nulls(rng, 777, 300), keys_with_nulls(rng, n, 300), 300, kind, where=("R", n, kind))


@pytest.mark.parametrize("G", [1, 2, 256, 257, 65536, 65537, 2**24 + 1])
def test_digit_borders(dev, jtw, G):
    """G at the borders of the 8-bit digits: one pass for G <= 256 (G = 1 included: the pass that leaves out the rows without a
    key), two up to 65 536, three up to 2^24, four above.  The keys come from a pool spread over all of [0, G), both ends in it"""
    rng = np.random.default_rng(G)
    pool = np.unique(np.concatenate([[0, G - 1, G // 2], rng.integers(0, G, 400)]))
    draw = lambda n: np.where(rng.random(n) < 0.1, -1, rng.choice(pool, n)).astype(np.int32)
    for kind in (INNER, LEFT):
        run_join(dev, jtw, draw(3000), draw(2600), G, kind, where=(G, kind))
    run_join(dev, jtw, draw(1500), draw(1500), G, SEMI, keys_capacity=G + 1000, where=(G, "room above G"))
    # every right row with a key in ONE bucket in every pass (a wave adds to the histogram once) and equal keys across every
    # wave, round and tile border: ascending r; rows without a key on both sides of a wave border and a tile border in pass 0
    one = np.full(2 * T + 1, G - 1, dtype=np.int32)
    one[[63, 64, T - 1, T]] = -1
    want, _ = run_join(dev, jtw, np.array([G - 1, -1, G - 1], dtype=np.int32), one, G, INNER, where=(G, "one bucket"))
    assert want.res.n_right_null == 4 and want.res.n_pairs == 2 * (2 * T - 3)
    # all the buckets of pass 0 inside one tile
    buckets = min(G, 256)
    run_join(dev, jtw, np.arange(buckets, dtype=np.int32), (np.arange(T) % buckets).astype(np.int32), G, INNER, where=(G, "every bucket"))


def test_hot_key(dev, jtw):
    """One key held by 3 000 left and 3 000 right rows among 20 000 others: 9 M pairs, each hot left row's 3 000 pairs crossing
    emit blocks (kTile = 1 024 pairs), the whole past jn_emit's 4 096 blocks"""
    rng = np.random.default_rng(1)
    def side():
        k = rng.integers(1, 50000, 23000, dtype=np.int64)
        k[rng.choice(23000, 3000, replace=False)] = 0
        return k.astype(np.int32)
    want, _ = run_join(dev, jtw, side(), side(), 50000, INNER)
    assert want.res.n_pairs > 9_000_000


@pytest.mark.parametrize("first", [1000, T, T + 24])
def test_rows_that_emit_nothing_across_an_emit_block(dev, jtw, first):
    """5 000 consecutive left rows without a partner between rows that have one: the stretch lies inside an emit block's row
    range (more than kStage = 1 025 offsets: the lanes search the global array), at its border, and just behind it"""
    lk = np.concatenate([np.arange(first), np.full(5000, -1), np.arange(2000)]).astype(np.int32)
    rk = np.arange(2000, dtype=np.int32)
    for kind in (INNER, SEMI):
        run_join(dev, jtw, lk, rk, 2000, kind, where=(first, kind))
    # ANTI: the rows WITH a partner are the stretch
    lk = np.concatenate([1000 + np.arange(first) % 1000, np.arange(5000) % 1000, 1000 + np.arange(2000) % 1000]).astype(np.int32)
    run_join(dev, jtw, lk, rk[:1000], 2000, ANTI, where=(first, "anti"))


def test_stability_across_tiles_and_wave_halves(dev, jtw):
    """Right rows of one key in four tiles and in both halves of a wave (lanes 5 and 40), with three digits so that every later
    pass has to keep the order of the one before"""
    G = 70000
    rk = (np.arange(4000, dtype=np.int64) * 17 + 1000) % G
    same = [5, 40, 70, T + 30, T + 100, 2 * T + 2, 2 * T + 90, 3 * T + 500]
    rk[same] = 66666
    rk[[6, 41, T + 31]] = 66666 + 256        # the same low digit
    lk = np.array([66666, 1000, 66666 + 256, 66666], dtype=np.int32)
    want, _ = run_join(dev, jtw, lk, rk.astype(np.int32), G, INNER)
    assert want.right[:8].tolist() == same and want.right[9:12].tolist() == [6, 41, T + 31]


@pytest.mark.parametrize("kind", KINDS)
def test_clipped_then_repeated(dev, jtw, kind):
    rng = np.random.default_rng(10 + kind)
    lk, rk = keys_with_nulls(rng, 2000, 90), keys_with_nulls(rng, 1500, 90)
    M = tjm.np_join(lk, rk, len(lk), len(rk), 90, kind)[3][0]
    want, _ = run_join(dev, jtw, lk, rk, 90, kind, pairs_capacity=M - 1, where="clipped")
    assert (want.res.code, want.res.n_pairs) == (MSJ_CAPACITY, M) and (want.left == FILL32).all()
    want, _ = run_join(dev, jtw, lk, rk, 90, kind, pairs_capacity=want.res.n_pairs, where="repeated")
    assert want.res.code == 0


@pytest.mark.parametrize("kind", KINDS)
def test_counts_on_the_device_only(dev, jtw, kind):
    """L, R and G given on the device, the host arguments at their rooms; poison keys behind L and R"""
    rng = np.random.default_rng(20 + kind)
    lk, rk = keys_with_nulls(rng, 5000, 1000), keys_with_nulls(rng, 4000, 1000)
    lk[3100:], rk[2900:] = POISON, 7
    run_join(dev, jtw, lk, rk, 10**6, kind, L=3100, R=2900, G_dev=1000, keys_capacity=10**6)
    for kw in (dict(L=5001), dict(R=4001), dict(G_dev=10**6 + 1), dict(L=2**31)):
        run_join(dev, jtw, lk, rk, 10**6, kind, keys_capacity=10**6, pairs_capacity=64, where=kw, **kw)


@pytest.mark.parametrize("how", ["inner", "left"])
def test_chain_from_two_dictionary_calls_to_taken_rows(dev, how):
    """dictionary_extend (right) -> dictionary_extend frozen (left) -> join -> take_rows on both sides, sync=False throughout:
    P, L, R and G pass from result to call on the device.  The taken records against a join of the json.loads rows in Python,
    the code-20 records of how="left" included"""
    import torch

    from mojo_simdjson_amd.document_stream import RowSelection
    from tests import test_join_documents as tjd

    events, users = tjd.events_and_users()
    ewin = next(tjd.windows_of(dev, events, ["/user", "/n"]))
    uwin = next(tjd.windows_of(dev, users, ["/id", "/name"]))
    (l_off, l_bytes, l_valid), (r_off, r_bytes, r_valid) = ewin.strings("/user"), uwin.strings("/id")
    cap, room = 256, 1024
    d_off = torch.zeros(cap + 1, dtype=torch.int64, device=dev.device)
    d_first = torch.zeros(cap, dtype=torch.int32, device=dev.device)
    d_bytes = torch.zeros(8192, dtype=torch.uint8, device=dev.device)
    word = lambda d_res, k: d_res[8 * k:8 * k + 8].view(torch.int64)      # n_rows: word 1; n_distinct: word 3
    r_res, r_codes, *_ = dev.dictionary_extend(r_off, r_bytes, r_valid.view(torch.uint8), d_off, d_first, d_bytes, rows=len(users), sync=False)
    l_res, l_codes, *_ = dev.dictionary_extend(l_off, l_bytes, l_valid.view(torch.uint8), d_off, d_first, d_bytes, d_n_prior=word(r_res, 3),
                                               rows=len(events), frozen=True, sync=False)
    d_res, d_l, d_r, _, d_lsel, d_rsel = dev.join_rows(l_codes, r_codes, d_n_keys=word(r_res, 3), keys_capacity=cap, how=how, d_n_left=word(l_res, 1),
                                                       d_n_right=word(r_res, 1), pairs_capacity=room, sync=False)
    _, l_out, l_osel = dev.take_rows(d_l, d_lsel, ewin.d_fields, ewin.d_select, out_capacity=room, sync=False)
    _, r_out, r_osel = dev.take_rows(d_r, d_rsel, uwin.d_fields, uwin.d_select, out_capacity=room, sync=False)
    torch.cuda.synchronize()
    res = _lib.MsjJoinRowsResult.from_buffer_copy(d_res.cpu().numpy().tobytes())
    want = tjd.py_join(events, users, "user", "id", how, tjd.string_key)
    M = len(want)
    assert (res.code, res.n_pairs, res.n_left, res.n_right) == (0, M, len(events), len(users)) and res.n_keys == len({u["id"] for u in users if isinstance(u.get("id"), str)})
    left = RowSelection(ewin, None, d_l[:M], l_out[:, :M], l_osel)
    right = RowSelection(uwin, None, d_r[:M], r_out[:, :M], r_osel)
    got = list(zip(zip(left.values("/user"), left.values("/n")), zip(right.values("/id"), right.values("/name"))))
    assert got == tjd.flat(want, ("user", "n"), ("id", "name"), True)
    codes = right.column("/name")["code"].tolist()
    assert codes == [0 if r is not None else 20 for _, r in want] and (how == "inner" or 20 in codes)


def test_argument_checks_on_the_entry_point(dev, jtw):
    """The entry point refuses what the twin refuses, with the same code, for the same pointers (the twin returns before it reads
    anything): the header's order -- NULLs, an unknown flag and overlapping offsets in front of the 2^40 rooms, those in front
    of alignment and a select result that is d_result.  Nothing is launched: the outputs keep their fill"""
    import torch

    held = Held(dev, np.arange(12, dtype=np.int32), np.arange(11, dtype=np.int32), 64)
    lk, rk, out, off, res, sel = (t.data_ptr() for t in (held.d_lk, held.d_rk, held.t_left, held.t_off, held.t_res, held.t_lsel))
    big = 1 << 40
    base = dict(ctx=1, left=lk, left_rows=12, n_left=None, right=rk, right_rows=11, keys_capacity=7, flags=0, out_left=out, out_right=None,
                pairs_capacity=4, offsets=None, result=res, lsel=None)
    cases = [dict(ctx=0), dict(result=None), dict(left=None), dict(right=None), dict(out_left=None), dict(flags=4), dict(flags=1 << 31),
             dict(offsets=lk), dict(offsets=rk - 8 * 12), dict(n_left=off, offsets=off)]
    cases += [dict(c, keys_capacity=big) for c in cases]
    for room in ("left_rows", "right_rows", "keys_capacity", "pairs_capacity"):
        cases += [{room: big}, {room: big, "out_right": out + 2}, {room: big, "lsel": res}]
    cases += [dict(left=lk + 2), dict(out_left=out + 2), dict(out_right=out + 1), dict(offsets=off + 4), dict(n_left=off + 4), dict(result=res + 4),
              dict(lsel=sel + 4), dict(lsel=res)]
    codes = set()
    for case in cases:
        a = dict(base, **case)
        args = (a["left"], a["left_rows"], a["n_left"], a["right"], a["right_rows"], None, 7, None, a["keys_capacity"], a["flags"], a["out_left"],
                a["out_right"], a["pairs_capacity"], a["offsets"], a["result"], a["lsel"], None)
        want = jtw.jrm_join_rows(a["ctx"], *args)
        got = dev.lib.msj_join_rows_device(dev.ctx if a["ctx"] else None, *args, dev._stream())
        assert got == want and want in (tjm.BAD_ARGUMENT, MSJ_CAPACITY), (case, got, want)
        codes.add(want)
    assert codes == {tjm.BAD_ARGUMENT, MSJ_CAPACITY}
    torch.cuda.synchronize()
    assert (held.t_left.cpu().numpy().view(np.uint32) == FILL32).all() and (held.t_res.cpu().numpy() == FILL).all()
