"""msj_dictionary_order_device and msj_rank_rows_device past their grids (csrc/dictionary_order_kernel.hip), in the manner of
tests/test_join_rows_scale.py: the smallest V at which every grid-strided kernel makes a second trip and every one-workgroup
scan takes a second chunk, whole tensors against the host twin, and the twin once against ``sorted``.

The borders, with the constant each comes from:
  V = 1 048 576 + 1 025   one tile and one entry past kTileBlocks = 1 024 blocks x kTile = 1 024 positions: every kernel over
                          tiles wraps; do_init_scan / do_tied_scan / do_scan / do_heads_scan: more than kScan = 1 024 tiles, so
                          the scans take a second chunk; three rank digits
  values id%07d           two rounds; the constant leading digits cost no pass
  the variant             4 200 entries share a 24-byte prefix: rounds 1 and 2 have nothing else tied, and the tied set of round
                          3 (4 200 entries, more than four tiles of tied entries) crosses tile borders
  R = 1 048 576 + 1       rr_rows: 4 096 blocks x 256 rows and one more
"""
import numpy as np
import pytest

from tests import test_dictionary_order as tdo
from tests import test_dictionary_order_math as tdm
from tests.test_dictionary_order import dev, tw  # noqa: F401

pytestmark = pytest.mark.gpu

V = 1024 * 1024 + 1025
SHARED = 4200
ROWS = 1024 * 1024 + 1


class FlatDict:
    """Every entry with a value, the values back to back: tdm.Dict's members without its per-entry Python"""

    def __init__(self, values):
        self.values, self.V = values, len(values)
        lengths = np.fromiter((len(v) for v in values), dtype=np.uint64, count=len(values))
        self.offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
        self.bytes = np.frombuffer(b"".join(values), dtype=np.uint8).copy()
        self.cap = int(self.bytes.size)


def ids(variant):
    rng = np.random.default_rng(12)
    vals = [b"id%07d" % i for i in rng.permutation(V)]
    if variant:
        for k, c in enumerate(rng.choice(V, SHARED, replace=False)):
            vals[c] = b"zone-a/rack-00/host-000/" + b"%04d" % ((k * 7919) % 10000)
    return vals


@pytest.mark.parametrize("variant", (False, True))
def test_past_every_grid(dev, tw, variant):  # noqa: F811
    vals = ids(variant)
    d = FlatDict(vals)
    rc, want, ws, wr, passes = tdm.run_twin(tw, d, max_rounds=8, mode=tdm.GRID)
    order = sorted(range(V), key=vals.__getitem__)   # (every value is distinct)
    assert rc == 0 and want.code == 0 and want.depth == (32 if variant else 16) and np.array_equal(ws, np.array(order, dtype=np.uint32))
    held = tdo.Held(dev, d)
    rc, got = held.call(tdm.AUTO, max_rounds=8)
    assert rc == 0 and tdo.fields(got[2]) == tdo.fields(bytes(want))
    tdo.check(got, want, ws, wr, V)
    if not variant:
        assert want.n_equal == 0 and np.array_equal(ws[wr], np.arange(V, dtype=np.uint32)) and passes == 6 + 1 + 3
        # rank_rows over one row more than its grid covers in a trip
        import torch

        rng = np.random.default_rng(5)
        codes = rng.integers(-2, V + 2, ROWS).astype(np.int32)
        rc, wres, wsel, wfields = tdm.run_rank_rows(tw, codes, wr, want)
        t_fields = torch.full((ROWS + tdo.CANARY, 2), 0xA5A5A5A5A5A5A5A5 - 2**64, dtype=torch.int64, device=dev.device)
        d_res, d_fields, d_sel = dev.rank_rows(tdo.to_dev(dev, codes), held.t_rank, held.t_res, rank_capacity=V, d_fields=t_fields, capacity=ROWS, sync=False)
        torch.cuda.synchronize()
        assert d_res.cpu().numpy().tobytes() == bytes(wres) and d_sel.cpu().numpy().tobytes() == bytes(wsel)
        assert t_fields.cpu().numpy().tobytes() == wfields.tobytes() + b"\xA5" * (16 * tdo.CANARY)
