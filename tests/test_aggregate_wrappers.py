"""The host side of ``stats`` (mojo_simdjson_amd/document_stream.py) without a GPU: what ``GroupStats`` makes of the
``msj_aggregate`` records -- here the host twin's, as CPU tensors -- and how a list column's offsets become a code per
element.  The argument checks of the C call, in the header's order, need a context: tests/test_aggregate.py::test_check_order."""
import ctypes
import math

import numpy as np
import torch

from mojo_simdjson_amd import _lib
from mojo_simdjson_amd.document_stream import GroupStats, _rows_of_elements
from tests import test_aggregate_math as tam


class Keys:
    def __init__(self, names):
        self.names = names

    def values(self):
        return self.names


def test_group_stats_views_and_python():
    atw = tam.load_twin()
    values = [tam.INT64_MAX, 2.5, 1, -0.0, tam.Raw(0, "n"), 1.7e308, -7, 1.7e308, 9007199254740993]
    codes = np.array([0, 1, 0, 1, 2, 3, 2, 3, -1], dtype=np.int32)
    cols = np.stack([tam.records(values), tam.records([1] * len(values))])
    a = tam.twin_aggregate(atw, cols, len(values), codes, 4)
    assert a.rc == 0 and a.res.code == 0
    stats = GroupStats(Keys(["a", "b", "c", "d"]), ["/x", "/one"], torch.from_numpy(a.groups.copy()).view(2, 4, 48), a.res)
    assert stats.n_groups == 4 and stats.n_ungrouped == 1 and stats.n_skipped == 0
    assert stats.n_rows.tolist() == [2, 2, 2, 2] and stats.n_values.tolist() == [[2, 2, 1, 2], [2, 2, 2, 2]]
    assert stats.sum_types.tolist() == [[tam.D, tam.D, tam.L, tam.D], [tam.L] * 4] and stats.sums[1].tolist() == [2, 2, 2, 2]
    assert stats.flags.tolist() == [[_lib.AGG_INT_OVERFLOW, 0, 0, _lib.AGG_INFINITE], [0] * 4]
    assert stats.mins[0, 2].item() == -7 and stats.min_types[0, 1].item() == tam.D and stats.maxs[0, 0].item() == tam.INT64_MAX
    got = stats.to_python()
    assert [g["key"] for g in got] == ["a", "b", "c", "d"]
    assert got[0]["/x"] == {"n_rows": 2, "n_values": 2, "sum": 9223372036854775808.0, "min": 1, "max": tam.INT64_MAX, "flags": 1}
    assert type(got[0]["/x"]["min"]) is int and type(got[0]["/x"]["sum"]) is float
    assert got[1]["/x"]["sum"] == 2.5 and math.copysign(1, got[1]["/x"]["min"]) < 0 and got[1]["/x"]["max"] == 2.5
    assert got[2]["/x"] == {"n_rows": 2, "n_values": 1, "sum": -7, "min": -7, "max": -7, "flags": 0}
    assert got[3]["/x"]["sum"] == math.inf and got[3]["/x"]["flags"] == _lib.AGG_INFINITE and got[3]["/one"]["sum"] == 2
    # no keys: no "key"; a group without a value: None
    b = tam.twin_aggregate(atw, tam.records([tam.Raw(0, "n")]), 1, None, 1)
    alone = GroupStats(None, [""], torch.from_numpy(b.groups.copy()).view(1, 1, 48), b.res).to_python()
    assert alone == [{"": {"n_rows": 1, "n_values": 0, "sum": None, "min": None, "max": None, "flags": 0}}]


def test_rows_of_elements():
    offsets = torch.tensor([0, 0, 3, 3, 4, 9, 9], dtype=torch.int64)
    assert _rows_of_elements(offsets, 9).tolist() == [1, 1, 1, 3, 4, 4, 4, 4, 4]
    assert _rows_of_elements(offsets, 9).dtype == torch.int32 and _rows_of_elements(torch.zeros(4, dtype=torch.int64), 0).tolist() == []


def test_structs():
    assert ctypes.sizeof(_lib.MsjAggregate) == 48 == tam.AGG_DTYPE.itemsize and ctypes.sizeof(_lib.MsjAggregateResult) == 48
    assert [(n, _lib.MsjAggregate.__dict__[n].offset) for n, _ in _lib.MsjAggregate._fields_] == \
        [(n, tam.AGG_DTYPE.fields[n][1]) for n in tam.AGG_DTYPE.names]
