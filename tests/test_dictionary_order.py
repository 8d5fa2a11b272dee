"""A dictionary's values in byte order on the device (msj_dictionary_order_device and msj_rank_rows_device,
csrc/dictionary_order_kernel.hip), through the C ABI.

Expected values come from the host twin of the same arithmetic (tests/dictionary_order_math_host.cpp), which
tests/test_dictionary_order_math.py holds against the definition written in Python, and from that definition itself
(``py_order``: ``sorted`` and ``bisect``; it shares nothing with the kernels).  Device output is compared with both over
WHOLE tensors: d_sorted and d_rank start from the fill 0xA5 with a canary behind the room, so a store at or past V shows;
the 48-byte results byte for byte.

The kernel's constants as the shapes use them: kTile = 1 024 positions or tied entries per block, which is also the most
entries of the one-workgroup path (so 1 023 / 1 024 / 1 025 are both borders), 8-bit digits.
"""
import numpy as np
import pytest

from tests import test_dictionary_order_math as tdm

pytestmark = pytest.mark.gpu

CANARY = 16
FILL32, NO_RANK = tdm.FILL32, tdm.NO_RANK
AUTO, GRID, GROUP = tdm.AUTO, tdm.GRID, tdm.GROUP
MSJ_CAPACITY, BAD_ARGUMENT, CONTINUE = 1, -1, 1


@pytest.fixture(scope="module")
def dev():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mojo_simdjson_amd.device import Stage1Device

    d = Stage1Device(0)
    yield d
    d.set_order_mode(AUTO)
    d.close()


@pytest.fixture(scope="module")
def tw():
    return tdm.load_twin()


def to_dev(dev, a):
    import torch

    a = np.ascontiguousarray(a)
    if a.size == 0:
        return torch.zeros((8,), dtype=torch.uint8, device=dev.device).view({1: torch.uint8, 4: torch.int32, 8: torch.int64}[a.itemsize])
    return torch.from_numpy(a.view({1: np.uint8, 4: np.int32, 8: np.int64}[a.itemsize]).copy()).to(dev.device)


class Held:
    """A dictionary and a call's outputs on the device, the outputs filled and with a canary behind the room"""

    def __init__(self, dev, d, capacity=None, misalign=0):
        import torch

        self.dev, self.d = dev, d
        self.capacity = d.V if capacity is None else capacity
        self.d_offsets = to_dev(dev, d.offsets)
        raw = torch.zeros((d.cap + misalign + 8,), dtype=torch.uint8, device=dev.device)
        raw[misalign:misalign + d.cap] = torch.from_numpy(d.bytes.copy()).to(dev.device)
        self.raw, self.bytes_ptr = raw, raw.data_ptr() + misalign
        self.t_sorted = torch.empty((self.capacity + CANARY,), dtype=torch.int32, device=dev.device)
        self.t_rank = torch.empty((self.capacity + CANARY,), dtype=torch.int32, device=dev.device)
        self.t_res = torch.empty((48,), dtype=torch.uint8, device=dev.device)
        self.refill()

    def refill(self):
        self.t_sorted.fill_(FILL32 - 2**32), self.t_rank.fill_(FILL32 - 2**32), self.t_res.fill_(0xA5)

    def call(self, mode, depth=0, max_rounds=0, flags=0, d_n_entries=None, n_entries=None, wait=True):
        import torch

        dev = self.dev
        dev.set_order_mode(mode)
        rc = dev.lib.msj_dictionary_order_device(dev.ctx, self.d_offsets.data_ptr(), self.bytes_ptr if self.d.cap else None, self.d.cap,
                                                 self.d.V if n_entries is None else n_entries, d_n_entries, self.capacity, depth, max_rounds,
                                                 flags, self.t_sorted.data_ptr(), self.t_rank.data_ptr(), self.t_res.data_ptr(), dev._stream())
        dev.set_order_mode(AUTO)
        if not wait or rc != 0:
            return rc
        torch.cuda.synchronize()
        return rc, self.out()

    def out(self):
        return self.t_sorted.cpu().numpy().view(np.uint32), self.t_rank.cpu().numpy().view(np.uint32), self.t_res.cpu().numpy().tobytes()


def with_canary(a, room):
    out = np.full(room + CANARY, FILL32, dtype=np.uint32)
    out[:len(a)] = a
    return out


def check(got, want_res, want_sorted, want_rank, capacity):
    srt, rnk, res = got
    assert res == bytes(want_res), (fields(res), fields(bytes(want_res)))
    assert (srt == with_canary(want_sorted, capacity)).all()
    assert (rnk == with_canary(want_rank, capacity)).all()


def fields(res):
    r = tdm.OrderResult.from_buffer_copy(res)
    return dict(code=r.code, flags=r.flags, V=r.n_entries, values=r.n_values, tied=r.n_tied, depth=r.depth, equal=r.n_equal)


def run_order(dev, tw, d, mode, capacity=None, max_rounds=64, misalign=0, definition=True):
    """One call on the device against the twin and the definition -> the twin's (result, sorted, rank)"""
    capacity = d.V if capacity is None else capacity
    rc, want, ws, wr, _ = tdm.run_twin(tw, d, capacity=capacity, max_rounds=max_rounds, mode=mode)
    assert rc == 0
    if definition:
        tdm.check_against(d.values, want, ws, wr, None if want.code == 0 else want.depth, capacity)
    held = Held(dev, d, capacity, misalign)
    rc, got = held.call(mode, max_rounds=max_rounds)
    assert rc == 0
    assert fields(got[2]) == fields(bytes(want))
    check(got, want, ws, wr, capacity)
    return want, ws, wr


@pytest.mark.parametrize("name", sorted(tdm.CORPUS))
def test_corpus_on_both_paths(dev, tw, name):
    d = tdm.Dict(tdm.CORPUS[name])
    for mode in (GRID, GROUP, AUTO):
        run_order(dev, tw, d, mode, misalign=len(name) % 8)


def test_past_a_tile_and_room_to_spare(dev, tw):
    import random

    rng = random.Random(2)
    for V in (2047, 2049, 3000):
        pre = tdm.word(rng, 11)
        vals = [None if rng.random() < 0.01 else pre + tdm.word(rng, rng.choice((0, 2, 5, 8, 13))) for _ in range(V)]
        run_order(dev, tw, tdm.Dict(vals), GRID, capacity=V + 7)
    small = tdm.Dict(tdm.CORPUS["prefix-9-holes"])
    run_order(dev, tw, small, AUTO, capacity=1024)
    run_order(dev, tw, small, AUTO, capacity=1025)


@pytest.mark.parametrize("budget", (1, 2))
@pytest.mark.parametrize("name", ("prefix-17-holes", "prefix-65", "equal-multiples-of-8", "border-1024"))
def test_continued_chains(dev, tw, name, budget):
    """Every call of a chain against the twin's; the first call on the one-workgroup path, the rest on the grid path"""
    d = tdm.Dict(tdm.CORPUS[name])
    _, want, want_s, want_r, _ = tdm.run_twin(tw, d, max_rounds=64, mode=GRID)
    held = Held(dev, d)
    state, depth, calls = None, 0, 0
    while True:
        mode = GROUP if calls == 0 else GRID
        flags = CONTINUE if calls else 0
        rc, res, srt, rnk, _ = tdm.run_twin(tw, d, depth=depth, max_rounds=budget, flags=flags, mode=mode, state=state)
        assert rc == 0
        rc, got = held.call(mode, depth=depth, max_rounds=budget, flags=flags)
        assert rc == 0
        assert fields(got[2]) == fields(bytes(res))
        check(got, res, srt, rnk, d.V)
        calls += 1
        if res.code == 0:
            break
        state, depth = (srt, rnk), res.depth
        assert calls < 40
    assert (srt == want_s).all() and (rnk == want_r).all() and res.n_equal == want.n_equal


def test_long_values(dev, tw):
    import random

    rng = random.Random(9)
    shared = tdm.word(rng, 520)
    vals = [shared + tdm.word(rng, rng.randrange(0, 30)) for _ in range(40)] + [b"a", b"", b"b" * 3, shared]
    long = bytes(rng.choice(tdm.ALPHABET) for _ in range(70000))
    vals += [long]
    rng.shuffle(vals)
    d = tdm.Dict(vals)
    for mode in (GROUP, GRID):
        # 520 shared bytes take 66 rounds: two calls of 64, each against the twin
        held = Held(dev, d)
        state, depth, calls = None, 0, 0
        while True:
            flags = CONTINUE if calls else 0
            rc, res, srt, rnk, _ = tdm.run_twin(tw, d, depth=depth, max_rounds=64, flags=flags, mode=mode, state=state)
            rc, got = held.call(mode, depth=depth, max_rounds=64, flags=flags)
            assert rc == 0 and fields(got[2]) == fields(bytes(res))
            check(got, res, srt, rnk, d.V)
            calls += 1
            if res.code == 0:
                break
            state, depth = (srt, rnk), res.depth
            assert calls < 200
        tdm.check_against(vals, res, srt, rnk, None, d.V)


def string_column(values):
    """(offsets, bytes, valid) of a column of rows; None is a null row"""
    offsets, data, valid = [0], bytearray(), []
    for v in values:
        data += v or b""
        offsets.append(len(data))
        valid.append(0 if v is None else 1)
    return np.array(offsets, dtype=np.uint64), np.frombuffer(bytes(data) or b"\x00", dtype=np.uint8), np.array(valid, dtype=np.uint8)


def test_behind_a_dictionary_call_then_rank_and_sort(dev, tw):
    """V read on the device behind a real msj_dictionary_device call with nothing waited for; d_sorted[d_rank[c]] == c; and
    rank_rows then msj_sort_rows_device is ``sorted`` over the rows' strings, None last, stable"""
    import random

    import torch

    rng = random.Random(4)
    pool = [b"host-%03d" % rng.randrange(400) for _ in range(300)] + [b"", b"host", b"host-\x00", b"host-\xff", b"Host-001"]
    rows = [None if rng.random() < 0.1 else rng.choice(pool) for _ in range(5000)]
    off, data, valid = string_column(rows)
    d_off, d_data, d_valid = to_dev(dev, off), to_dev(dev, data), to_dev(dev, valid)
    room = 1500
    for mode in (GRID, GROUP):
        cap = room if mode == GRID else 1024
        d_res, d_codes, d_do, d_df, d_db = dev.dictionary(d_off, d_data, d_valid, rows=len(rows), dict_capacity=cap, dict_bytes_capacity=1 << 16,
                                                          sync=False)
        dev.set_order_mode(mode)
        d_ores, d_sorted, d_rank = dev.dictionary_order(d_do, d_db, d_n_entries=d_res[24:32].view(torch.int64), capacity=cap, max_rounds=8, sync=False)
        dev.set_order_mode(AUTO)
        d_rres, d_fields, d_sel = dev.rank_rows(d_codes, d_rank, d_ores, sync=False)
        sres, d_order, _ = dev.sort_rows(d_fields, d_sel)
        torch.cuda.synchronize()
        ores = fields(d_ores.cpu().numpy().tobytes())
        V = ores["V"]
        distinct = sorted(set(r for r in rows if r is not None))
        assert (ores["code"], V, ores["values"], ores["tied"], ores["equal"]) == (0, len(distinct), len(distinct), 0, 0)
        do, db = d_do.cpu().numpy(), d_db.cpu().numpy().tobytes()
        srt, rnk = d_sorted.cpu().numpy()[:V], d_rank.cpu().numpy()[:V]
        assert [db[do[e]:do[e + 1]] for e in srt] == distinct
        assert (srt[rnk] == np.arange(V)).all()
        rres = tdm.RankRowsResult.from_buffer_copy(d_rres.cpu().numpy().tobytes())
        n_null = sum(r is None for r in rows)
        assert (rres.code, rres.n_rows, rres.n_ranked, rres.n_null, rres.n_unknown) == (0, len(rows), len(rows) - n_null, n_null, 0)
        want = sorted(range(len(rows)), key=lambda k: (rows[k] is None, rows[k] or b"", k))
        assert sres.code == 0 and list(d_order.cpu().numpy()[:len(rows)]) == want


def test_rank_rows_whole_tensors(dev, tw):
    import torch

    vals = [b"pear", None, b"apple", b"fig", b"apple"]
    d = tdm.Dict(vals)
    _, order, srt, rnk, _ = tdm.run_twin(tw, d, max_rounds=64)
    codes = np.array([0, 2, -1, -2, 5, 1, 3, 4, 2, 1 << 30, -(1 << 31)] * 100, dtype=np.int32)
    d_codes, d_rank = to_dev(dev, codes), to_dev(dev, rnk)
    d_order = torch.from_numpy(np.frombuffer(bytes(order), dtype=np.uint8).copy()).to(dev.device)
    tied = tdm.OrderResult.from_buffer_copy(bytes(order))
    tied.code, tied.n_tied = MSJ_CAPACITY, 2
    d_tied = torch.from_numpy(np.frombuffer(bytes(tied), dtype=np.uint8).copy()).to(dev.device)
    for kw, d_o, o in ((dict(n_rows=len(codes) - 1, capacity=len(codes) + 2), d_order, order), (dict(), d_tied, tied),
                       (dict(n_rows=len(codes) + 1), d_order, order), (dict(capacity=len(codes) - 1), d_order, order),
                       (dict(rank_capacity=d.V - 1), d_order, order)):
        rc, wres, wsel, wfields = tdm.run_rank_rows(tw, codes, rnk, o, **kw)
        assert rc == 0
        capacity = kw.get("capacity", len(codes))
        t_fields = torch.full((capacity + CANARY, 2), 0xA5A5A5A5A5A5A5A5 - 2**64, dtype=torch.int64, device=dev.device)
        t_res, t_sel = torch.full((48,), 0xA5, dtype=torch.uint8, device=dev.device), torch.full((48,), 0xA5, dtype=torch.uint8, device=dev.device)
        d_n = None if "n_rows" not in kw else torch.tensor([kw["n_rows"]], dtype=torch.int64, device=dev.device)
        rc = dev.lib.msj_rank_rows_device(dev.ctx, d_codes.data_ptr(), len(codes), None if d_n is None else d_n.data_ptr(), d_rank.data_ptr(),
                                          kw.get("rank_capacity", d.V), d_o.data_ptr(), t_fields.data_ptr(), capacity, t_res.data_ptr(),
                                          t_sel.data_ptr(), dev._stream())
        assert rc == 0
        torch.cuda.synchronize()
        assert t_res.cpu().numpy().tobytes() == bytes(wres) and t_sel.cpu().numpy().tobytes() == bytes(wsel)
        assert t_fields.cpu().numpy().tobytes() == wfields.tobytes() + b"\xA5" * (16 * CANARY)


def test_argument_checks_launch_nothing(dev, tw):
    import torch

    d = tdm.Dict([b"b", b"a", b"c"])
    held = Held(dev, d)
    lib, ctx, s = dev.lib, dev.ctx, dev._stream()
    o, b, srt, rnk, res = held.d_offsets.data_ptr(), held.bytes_ptr, held.t_sorted.data_ptr(), held.t_rank.data_ptr(), held.t_res.data_ptr()
    call = lib.msj_dictionary_order_device
    bad = [call(None, o, b, d.cap, 3, None, 3, 0, 0, 0, srt, rnk, res, s), call(ctx, o, b, d.cap, 3, None, 3, 0, 0, 0, srt, rnk, None, s),
           call(ctx, None, b, d.cap, 3, None, 3, 0, 0, 0, srt, rnk, res, s), call(ctx, o, b, d.cap, 3, None, 3, 0, 0, 0, None, rnk, res, s),
           call(ctx, o, b, d.cap, 3, None, 3, 0, 0, 0, srt, None, res, s), call(ctx, o, None, d.cap, 3, None, 3, 0, 0, 0, srt, rnk, res, s),
           call(ctx, o, b, d.cap, 3, None, 3, 0, 0, 2, srt, rnk, res, s), call(ctx, o, b, d.cap, 3, None, 3, 0, 65, 0, srt, rnk, res, s),
           call(ctx, o, b, d.cap, 3, None, 3, 4, 0, CONTINUE, srt, rnk, res, s), call(ctx, o, b, d.cap, 3, None, 3, 8, 0, 0, srt, rnk, res, s),
           call(ctx, o + 4, b, d.cap, 3, None, 3, 0, 0, 0, srt, rnk, res, s), call(ctx, o, b, d.cap, 3, o + 4, 3, 0, 0, 0, srt, rnk, res, s),
           call(ctx, o, b, d.cap, 3, None, 3, 0, 0, 0, srt + 2, rnk, res, s), call(ctx, o, b, d.cap, 3, None, 3, 0, 0, 0, srt, rnk + 1, res, s),
           call(ctx, o, b, d.cap, 3, None, 3, 0, 0, 0, srt, rnk, res + 4, s)]
    assert bad == [BAD_ARGUMENT] * len(bad)
    assert call(ctx, o, b, d.cap, 3, None, 1 << 40, 0, 0, 0, srt, rnk, res, s) == MSJ_CAPACITY
    assert call(ctx, o, b, d.cap, 3, None, 1 << 40, 0, 0, 2, srt, rnk, res, s) == BAD_ARGUMENT  # the flag is checked first
    assert dev.lib.msj_debug_set_order_mode(ctx, 3) == BAD_ARGUMENT
    torch.cuda.synchronize()
    got = held.out()
    assert (got[0] == FILL32).all() and (got[1] == FILL32).all() and got[2] == b"\xA5" * 48
    # V past the room, read on the device: the result alone
    d_n = torch.tensor([4], dtype=torch.int64, device=dev.device)
    for mode in (GRID, GROUP):
        held.refill()
        rc, got = held.call(mode, d_n_entries=d_n.data_ptr(), n_entries=0)
        assert rc == 0 and fields(got[2]) == dict(code=MSJ_CAPACITY, flags=0, V=4, values=0, tied=0, depth=0, equal=0)
        assert (got[0] == FILL32).all() and (got[1] == FILL32).all()
