"""msj_bucket_rows_device and msj_group_keys_device in stream order (the manner of tests/test_cast_strings_stream_order.py; the
delay and its bounds are tests/test_stream_order.py's): on a side stream, behind inputs that arrive late, with sync=False, the
capacity given and every output a tensor of the caller's.

The decoy B -- A's sizes, other numbers and codes -- lies in the records and the codes, and has been through both calls: every
tensor and the workspaces hold B's consistent state.  Then, on a side stream: a delay, device-to-device copies of A's records
and codes over them, the outputs back to their fill, and the two calls.  A launch or a memset that dropped its stream argument
runs ahead of the copies and reads the decoy; what it writes is then overwritten with the fill or differs from A's expected
arrays, which come from the host twin (tests/group_keys_math_host.cpp) alone.

What nullptr for `stream` would show, by the order of the checks below (reasoned from the launchers, not tried on a device):
at msj_launch_bucket_rows the kernels run on the null stream ahead of the side stream's copies and of its reset of the
outputs, so the array "out" fails first, at record 0, holding the fill where A's buckets belong ("res" and "osel" likewise); at
msj_launch_group_keys the same holds for "offsets", which is checked first of its arrays and fails at entry 0, and then for
"valid", "bytes" and "kres".
"""
import numpy as np
import pytest

from mojo_simdjson_amd import _lib
from tests import test_group_keys_math as tgm
from tests import test_stream_order as tso
from tests import test_tape_documents as ttd

ROWS = 2000
WIDTH, ORIGIN = 60000, -5
FLAGS = (0, tgm.NULL_IS_GROUP, 0)
W = 11 + 5 + 11


class Expected:
    """The two calls over one set of columns on the host: a bucket out of place, and keys from (the records, the codes, the
    buckets as the twin gives them)"""

    def __init__(self, decoy):
        gtw = tgm.load_twin()
        k = np.arange(ROWS, dtype=np.int64)
        values = (k * 7919 + (13 if decoy else 0)) % 1000003 - 500000
        self.records = tgm.records([int(v) if i % 3 else float(v) / 4 for i, v in enumerate(values)])
        self.records["token"] = k
        self.records["code"][(6 if decoy else 5)::17] = 20
        self.codes = ((k * (31 if decoy else 29)) % 97 - 1).astype(np.int32)
        self.rows = ROWS
        self.bucket = tgm.twin_bucket(gtw, self.records, ROWS, WIDTH, ORIGIN)
        parts = [tgm.Part(self.records, FLAGS[0]), tgm.Part(self.codes, FLAGS[1]), tgm.Part(self.bucket.out, FLAGS[2])]
        self.keys = tgm.twin_keys(gtw, parts, ROWS)
        assert self.bucket.rc == 0 and self.bucket.res.code == 0 and self.keys.rc == 0 and self.keys.res.code == 0
        assert min(self.bucket.res.n_bucketed, self.keys.res.n_keys, self.keys.res.n_null_rows) > 50

    def arrays(self):
        """{name: the expected bytes}, in the order they are checked"""
        struct = lambda s: np.frombuffer(bytes(s), dtype=np.uint8)
        raw = lambda x: np.frombuffer(np.ascontiguousarray(x).tobytes(), dtype=np.uint8)
        return {"out": raw(self.bucket.out), "res": struct(self.bucket.res), "osel": struct(self.bucket.out_sel),
                "offsets": raw(self.keys.offsets), "valid": raw(self.keys.valid), "bytes": raw(self.keys.bytes), "kres": struct(self.keys.res)}


def test_expected_on_cpu():
    """A's and the decoy's expected arrays have the same sizes and differ in the records and the key bytes: a call that read
    the decoy shows"""
    a, b = Expected(False), Expected(True)
    for name, want in a.arrays().items():
        other = b.arrays()[name]
        assert want.size == other.size and (name not in ("out", "bytes", "valid") or not np.array_equal(want, other)), name


class Tensors:
    """The inputs and the caller's output tensors of the two calls on one device"""

    def __init__(self, dev, x, start):
        import torch

        self.dev, self.x = dev, x
        self.d_rec = ttd.to_device(dev, start.records).view(torch.int64).view(-1, 2)
        self.d_codes = ttd.to_device(dev, start.codes)
        self.d_sel = ttd.to_device(dev, np.frombuffer(bytes(tgm.select_result(x.rows)), dtype=np.uint8))
        self.out = {name: ttd.to_device(dev, np.full(w.size, tgm.FILL, dtype=np.uint8)) for name, w in x.arrays().items()}
        self.pristine = {name: t.clone() for name, t in self.out.items()}

    def reset(self):
        for name, t in self.out.items():
            t.copy_(self.pristine[name], non_blocking=True)

    def call(self):
        import torch

        rows, o = self.x.rows, self.out
        d_out = o["out"].view(torch.int64).view(rows, 2)
        self.dev.bucket_rows(self.d_rec, self.d_sel, WIDTH, ORIGIN, capacity=rows, d_out=d_out, d_result=o["res"], d_out_select=o["osel"], sync=False)
        self.dev.group_keys([(self.d_rec, FLAGS[0]), (self.d_codes, FLAGS[1]), (d_out, FLAGS[2])], self.d_sel, capacity=rows,
                            d_offsets=o["offsets"].view(torch.int64), d_valid=o["valid"], d_bytes=o["bytes"], d_result=o["kres"], sync=False)

    def check(self, want, where):
        for name, w in want.items():
            got = self.out[name].cpu().numpy()
            bad = np.nonzero(got != w)[0]
            assert bad.size == 0, (where, name, int(bad[0]), got[bad[:4]].tolist(), w[bad[:4]].tolist(), int(bad.size))


@pytest.mark.gpu
def test_calls_behind_late_inputs(dev):
    import time

    import torch

    a, b = Expected(False), Expected(True)
    t = Tensors(dev, a, b)
    d_rec_a, d_codes_a = ttd.to_device(dev, a.records).view(torch.int64).view(-1, 2), ttd.to_device(dev, a.codes)

    def enqueue():
        t.reset()
        t.call()

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    enqueue()   # the decoy through the calls: the workspaces have their size and hold its state
    t_enq = time.perf_counter() - t0
    torch.cuda.synchronize()
    t.check(b.arrays(), "the decoy")
    s = torch.cuda.Stream(dev.device)
    need_ms = max(tso.MIN_DELAY_MS, tso.JITTER * t_enq * 1e3)
    start, ready = tso.delayed(s, need_ms), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(s):
        t.d_rec.copy_(d_rec_a, non_blocking=True)
        t.d_codes.copy_(d_codes_a, non_blocking=True)
        ready.record()
        enqueue()
    pending = not ready.query()
    s.synchronize()
    delay_ms = start.elapsed_time(ready)
    numbers = f"the enqueue took {t_enq * 1e3:.2f} ms on the host, the delay {delay_ms:.1f} ms of the {need_ms:.1f} ms it has to last"
    print(numbers)
    assert pending, "inconclusive: the inputs were there when the enqueue returned -- a host wait in the call, or the delay too short: " + numbers
    assert delay_ms >= need_ms, numbers
    t.check(a.arrays(), "behind late inputs")
    assert _lib.MsjGroupKeysResult.from_buffer_copy(t.out["kres"].cpu().numpy().tobytes()).n_keys == a.keys.res.n_keys


@pytest.fixture(scope="module")
def dev():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mojo_simdjson_amd.device import Stage1Device

    d = Stage1Device(0)
    yield d
    d.close()
