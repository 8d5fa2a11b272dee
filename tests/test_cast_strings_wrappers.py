"""The host side of ``where(..., cast=...)`` (mojo_simdjson_amd/document_stream.py) without a GPU: a ``datetime.datetime``
operand becomes its column's unit by integer arithmetic -- aware, or naive, which means UTC; never through a float -- and a
cast is named "number", "timestamp" or ("timestamp", unit)."""
import datetime

import pytest

from mojo_simdjson_amd.document_stream import _cast_spec, datetime_units
from tests.test_cast_strings_math import CAST, py_timestamp


def test_datetime_units():
    utc = datetime.timezone.utc
    ist = datetime.timezone(datetime.timedelta(hours=5, minutes=30))
    when = datetime.datetime(2024, 5, 1, 12, 34, 56, 789012, tzinfo=utc)
    assert datetime_units(when, "s") == 1714566896 and datetime_units(when, "ms") == 1714566896789
    assert datetime_units(when, "us") == 1714566896789012 and datetime_units(when, "ns") == 1714566896789012000
    assert datetime_units(when.replace(tzinfo=None), "us") == 1714566896789012
    assert datetime_units(datetime.datetime(2024, 5, 1, 18, 4, 56, 789012, tzinfo=ist), "us") == 1714566896789012
    # below the epoch the cut is a floor, as the call's is
    before = datetime.datetime(1969, 12, 31, 23, 59, 59, 999999)
    assert datetime_units(before, "us") == -1 and datetime_units(before, "ms") == -1 and datetime_units(before, "s") == -1
    # beyond 2^53 microseconds a float would round: the edges of datetime itself, against the yardstick of the cast
    for dt in (datetime.datetime.min, datetime.datetime.max, datetime.datetime(9999, 12, 31, 23, 59, 59, 999999, tzinfo=utc)):
        text = dt.replace(tzinfo=None).isoformat().encode() + b"Z"
        for unit in ("s", "ms", "us"):
            o, bits = py_timestamp(text, unit)
            assert o == CAST and datetime_units(dt, unit) == (bits - (1 << 64) if bits >> 63 else bits), (dt, unit)
    assert datetime_units(datetime.datetime.max, "us") == 253402300799999999 > 1 << 53


def test_cast_spec():
    assert _cast_spec("number") == ("number", "ns") and _cast_spec("timestamp") == ("timestamp", "ns")
    assert _cast_spec(("timestamp", "ms")) == ("timestamp", "ms") and _cast_spec(["timestamp", "s"]) == ("timestamp", "s")
    for bad in ("date", ("timestamp", "h"), ("number", "x")):
        with pytest.raises(ValueError):
            _cast_spec(bad)
