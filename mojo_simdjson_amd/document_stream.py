"""Multi-document mode: windows over a device-resident stream of concatenated JSON documents.

The reference parses one document per call and marks streaming as to do
(``src/mojo_simdjson/generic/stage2/tape_builder.mojo:25``; the hooks of upstream simdjson's
``stage1_mode::streaming_partial`` are visible in ``generic/stage1/json_structural_indexer.mojo:153,169``).
Upstream's ``document_stream`` cuts the input into batches, indexes each batch, walks the structurals
backwards to find where the last complete document ends and starts the next batch there.  Here the
same happens with three device passes per window -- stage 1 over the window (nothing is an error yet at
its end), the token pre-pass (type byte and depth per structural), the document split (a document
starts at every depth-0 token that is not a closing bracket) -- and the host only reads two small
result structs per window.

Every window starts at a document.  Stage 1 wants a 16-byte aligned base, so the window's base is
the document's offset rounded down and the up to 15 bytes in front (the end of the previous document)
read as blanks (``MSJ_FLAG_SKIP``).  Offsets in ``d_idx`` are relative to ``Window.base``.
"""
import datetime
import json
import struct
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _lib, errors
from .document import Document

DOC_TAPE_DTYPE = np.dtype([("tape_first", "<u8"), ("string_first", "<u8"), ("tape_words", "<u4"), ("code", "<i4"),
                           ("string_bytes", "<u8")])  # msj_document_tape
FIELD_DTYPE = np.dtype([("bits", "<u8"), ("token", "<u4"), ("type", "u1"), ("flags", "u1"), ("code", "<u2")])  # msj_field

MAX_WINDOW = 1 << 31


def _first_wins(pairs):
    out = {}
    for key, value in pairs:
        out.setdefault(key, value)
    return out


# a selected container's text: duplicate keys as the lookup itself treats them (at_key: the first one wins)
_CONTAINER = json.JSONDecoder(object_pairs_hook=_first_wins)
_ATOMS = {ord("t"): True, ord("f"): False, ord("n"): None}


def field_value(rec, data, idx, end):
    """The Python value of one ``msj_field`` (a FIELD_DTYPE row): None when it has a code; a string decoded from the
    window's bytes `data` (through json when it is escaped), a container from its text (its closing bracket is token
    rec["bits"]), a number from its bits -- or from its text when the record has none (MSJ_FIELD_NO_BITS).  idx, end: host
    copies of the window's d_idx / d_end."""
    if rec["code"] != 0:
        return None
    t, bits = int(rec["type"]), int(rec["bits"])
    if t in _ATOMS:
        return _ATOMS[t]
    if t == ord('"'):
        raw = bytes(data[bits & 0xFFFFFFFF:(bits & 0xFFFFFFFF) + (bits >> 32)])
        return json.loads(b'"' + raw + b'"') if rec["flags"] & 2 else raw.decode("utf-8")
    if t in (ord("{"), ord("[")):
        return _CONTAINER.decode(bytes(data[int(idx[int(rec["token"])]):int(idx[bits]) + 1]).decode("utf-8"))
    if t in (ord("l"), ord("d")):
        if rec["flags"] & _lib.FIELD_NO_BITS:
            v = int(rec["token"])
            return json.loads(bytes(data[int(idx[v]):int(end[v])]))
        return struct.unpack("<q" if t == ord("l") else "<d", struct.pack("<Q", bits))[0]
    raise ValueError(f"not a tape tag: {t}")


def number_column(col, dtype=torch.float64):
    """The numbers among ``msj_field`` records (int64 of shape (rows, 2)) as a column ON THE DEVICE, from the records alone
    (torch operations, no call): (values dtype[rows], valid bool[rows]).  torch.int64: valid where the value is an integer
    (tag 'l'); torch.float64: the doubles (tag 'd') as they are and the integers converted.  A number without bits
    (MSJ_FIELD_NO_BITS), a value of another kind and a record with a code are not valid; their value is 0."""
    if dtype not in (torch.int64, torch.float64):
        raise ValueError("dtype must be torch.int64 or torch.float64")
    bits, meta = col[:, 0].contiguous(), col[:, 1]
    tag, flags, code = (meta >> 32) & 0xFF, (meta >> 40) & 0xFF, (meta >> 48) & 0xFFFF
    has_bits = (code == 0) & ((flags & _lib.FIELD_NO_BITS) == 0)
    is_int, is_double = has_bits & (tag == ord("l")), has_bits & (tag == ord("d"))
    if dtype == torch.int64:
        return torch.where(is_int, bits, torch.zeros_like(bits)), is_int
    values = torch.where(is_double, bits.view(torch.float64), bits.to(torch.float64))
    valid = is_int | is_double
    return torch.where(valid, values, torch.zeros_like(values)), valid


def _or_blank(t, rows):
    """t, or where there is no row one blank row in its place: a call takes no empty array.  The rows are the last axis but
    one of records -- [rows, 2], [n_columns, rows, 2] -- and the only axis of a vector."""
    if rows:
        return t
    shape = list(t.shape)
    shape[max(t.dim() - 2, 0)] = 1
    return torch.zeros(shape, dtype=t.dtype, device=t.device)


def _code(d_result):
    """The code word of a result left on the device: the one read that waits for the call"""
    return int(d_result[:4].view(torch.int32).item())


# The helpers below take (the Window, records int64[rows, 2] or [n_columns, rows, 2], the device msj_select_documents_result
# that counts them, rows, ...) and `what`: the records' name, which a message puts behind "window at {base}:".

def _grow_once(window, call, d_rows, rows, room, total, what):
    """A column call over `rows` records whose output buffer starts from a guess of `room` items and, when the call says it
    was too small, is made as large as the call asks (the result field `total`) once.  call(d_rows, room, **outputs) is the
    ``Stage1Device`` method with everything else bound; outputs: d_offsets int64[rows + 1], d_valid uint8[rows] and the
    capacity, made here; d_rows: the records, or the fields whose column holds them.
    -> (result, what the call returned behind d_valid, offsets, valid bool[rows]); DocumentStreamError for a code"""
    d_rows, dvc = _or_blank(d_rows, rows), d_rows.device
    d_off = torch.empty(rows + 1, dtype=torch.int64, device=dvc)
    d_valid = torch.empty(max(rows, 1), dtype=torch.uint8, device=dvc)
    for _ in range(2):
        res, _, _, *out = call(d_rows, room, d_offsets=d_off, d_valid=d_valid, capacity=rows)
        if res.code != errors.CAPACITY or res.n_rows > rows:
            break
        room = int(getattr(res, total))
    if res.code != 0:
        raise DocumentStreamError(int(res.code), f"window at {window.base}: {what} could not be laid out")
    return res, out, d_off, d_valid[:rows].view(torch.bool)


def _string_column(window, d_fields, d_select, rows, p, bytes_capacity, what):
    """``string_column`` over `rows` records of column p of d_fields, its byte buffer grown once (``_grow_once``)
    -> (offsets int64[rows + 1], bytes uint8[total], valid bool[rows])"""
    w = window
    room = min(w.length, 32 * rows + 4096) if bytes_capacity is None else int(bytes_capacity)
    res, (d_bytes,), d_off, valid = _grow_once(
        w, lambda d_f, room, **out: w.dev.string_column(w.d_window, w.length, d_f, p, d_select, bytes_capacity=room, **out),
        d_fields, rows, room, "total_bytes", f"the strings of {what}")
    return d_off, d_bytes[:int(res.total_bytes)], valid


def _raw_column(window, d_rows, d_select, rows, compact, bytes_capacity, what):
    """``raw_column`` over `rows` records, its byte buffer grown once (``_grow_once``)
    -> (offsets int64[rows + 1], bytes uint8[total], valid bool[rows])"""
    w = window
    room = min(w.length, 64 * rows + 4096) if bytes_capacity is None else int(bytes_capacity)
    res, (d_bytes,), d_off, valid = _grow_once(
        w, lambda d_r, room, **out: w.dev.raw_column(w.d_window, w.length, w.d_idx, w.n_tokens, w.d_type, w.d_match, w.d_end, w.d_flags, d_r,
                                                     d_select, bytes_capacity=room, compact=compact, **out),
        d_rows, rows, room, "total_bytes", f"the text of {what}")
    return d_off, d_bytes[:int(res.total_bytes)], valid


def _array_elements(window, d_rows, d_select, rows, elements_capacity, parent, what, call=None):
    """``array_elements`` over `rows` records -- or call(d_rows, **outputs), ``Window.elements``' call over the documents --
    its element buffer grown once (``_grow_once``) -> ``ListColumn`` with `parent`"""
    w = window
    if call is None:
        call = lambda d_r, **out: w.dev.array_elements(*w._token_arrays(), d_r, d_select, **w._number_records(), **out)
    room = min(w.n_tokens, 4 * rows + 4096) if elements_capacity is None else int(elements_capacity)
    res, (d_elements, d_esel), d_off, valid = _grow_once(w, lambda d_r, room, **out: call(d_r, elements_capacity=room, **out),
                                                         d_rows, rows, room, "n_elements", f"the arrays of {what}")
    return ListColumn(w, d_off, d_elements[:int(res.n_elements)], valid, d_esel, parent)


def _object_entries(window, d_rows, d_select, rows, entries_capacity, parent, what):
    """``object_entries`` over `rows` records, its key and value buffers grown once (``_grow_once``) -> ``MapColumn`` with
    `parent`"""
    w = window
    room = min(w.n_tokens, 4 * rows + 4096) if entries_capacity is None else int(entries_capacity)
    res, (d_keys, d_values, d_ksel, d_vsel), d_off, valid = _grow_once(
        w, lambda d_r, room, **out: w.dev.object_entries(*w._token_arrays(), d_r, d_select, **w._number_records(), entries_capacity=room, **out),
        d_rows, rows, room, "n_entries", f"the objects of {what}")
    n = int(res.n_entries)
    return MapColumn(w, d_off, valid, d_keys[:n], d_values[:n], d_ksel, d_vsel, parent)


def _column_specs(specs, index):
    """Predicate specs whose columns are named by pointer or index -> the specs ``Stage1Device.compile_predicates`` takes;
    index: what turns a name into the column's number"""
    def one(spec):
        spec = tuple(spec)
        if len(spec) == 2 and spec[0] == "not":
            return ("not", one(spec[1]))
        return (index(spec[0]),) + spec[1:]

    return [one(s) for s in specs]


def _select_word(dvc, n):
    """A ``msj_select_documents_result`` on the device that counts n records of one column"""
    return torch.tensor(list(bytes(_lib.MsjSelectDocumentsResult(0, 0, int(n), 1, int(n), 0, 0))), dtype=torch.uint8, device=dvc)


def _take(window, d_fields, d_select, d_take, d_take_select, n_take, what):
    """``take_rows`` of n_take row numbers from d_fields (int64[n_columns, rows, 2]; from no row, every index is out of range)
    -> (fields int64[n_columns, n_take, 2], the uint8[48] select result that goes with them)"""
    d_res, d_out, d_out_select = window.dev.take_rows(d_take, d_take_select, _or_blank(d_fields, d_fields.shape[1]), d_select,
                                                      out_capacity=n_take, sync=False)
    code = _code(d_res)
    if code != 0:
        raise DocumentStreamError(code, f"window at {window.base}: {what} could not be taken")
    return d_out[:, :n_take], d_out_select


def _filter(window, d_fields, d_select, rows, specs, any, what, d_list_offsets=None):
    """``filter_rows`` over `rows` records per column of d_fields (int64[n_columns, rows, 2]) -> (keep bool[rows], kept
    int32[n_kept], the uint8[48] select result that counts them, the re-based list offsets or None).  The predicates live for
    the call; its 48-byte result comes to the host, which sizes what follows by n_kept."""
    w = window
    predicates = w.dev.compile_predicates(specs, any=any)
    try:
        res, d_keep, d_kept, d_kept_select, d_list_out = w.dev.filter_rows(predicates, w.d_window, w.length, _or_blank(d_fields, rows), d_select,
                                                                           capacity=rows, d_list_offsets=d_list_offsets)
    finally:
        predicates.close()
        w.dev._paths.remove(predicates)
    if res.code != 0 or res.n_rows != rows:
        raise DocumentStreamError(int(res.code), f"window at {w.base}: {what} could not be filtered")
    return d_keep[:rows].view(torch.bool), d_kept[:int(res.n_kept)], d_kept_select, d_list_out


# where's substring operators -> (the pattern's flags besides "nocase", is the operand LIKE text)
_MATCH_OPS = {"contains": ((), False), "suffix": (("at_end",), False), "like": ((), True)}


def _match_pattern(op, operand):
    """The operand of a ``where`` operator "contains" "suffix" "like" or their "i..." forms -> the pattern spec
    ``Stage1Device.compile_patterns`` takes, or None when `op` is none of them.  LIKE text: % separates the pieces, a leading
    or trailing % lifts that end's anchor; _ and an empty piece are refused"""
    nocase = op.startswith("i") and op[1:] in _MATCH_OPS
    name = op[1:] if nocase else op
    if name not in _MATCH_OPS:
        return None
    if not isinstance(operand, (str, bytes)):
        raise ValueError(f"the operand of {op!r} is a str or bytes: {operand!r}")
    data = operand.encode("utf-8") if isinstance(operand, str) else bytes(operand)
    flags, like = _MATCH_OPS[name]
    flags = set(flags) | ({"nocase"} if nocase else set())
    if not like:
        if not data:
            raise ValueError(f"the operand of {op!r} is not empty")
        return ([data], flags)
    if b"_" in data:
        raise ValueError(f"'like' has % only, no _: {operand!r}")
    pieces = data.split(b"%")
    if len(pieces) == 1 or pieces[0]:
        flags.add("at_start")
    if len(pieces) == 1 or pieces[-1]:
        flags.add("at_end")
    pieces = pieces[1 if not pieces[0] and len(pieces) > 1 else 0:]
    pieces = pieces[:-1] if pieces and not pieces[-1] else pieces
    if not pieces or any(not x for x in pieces):
        raise ValueError(f"'like' has no empty piece: {operand!r}")
    return (pieces, flags)


def _match_specs(specs, n_columns):
    """Predicate specs by column number with the substring operators rewritten: such a spec becomes (column, "found") on a
    new column behind the n_columns there are, which is to hold the match records of its pattern.
    -> (specs, {column: [(new column, pattern spec), ...]})"""
    wanted = {}
    count = [n_columns]

    def one(spec):
        if len(spec) == 2 and spec[0] == "not":
            return ("not", one(spec[1]))
        pattern = _match_pattern(spec[1], spec[2]) if len(spec) == 3 and isinstance(spec[1], str) else None
        if pattern is None:
            return spec
        wanted.setdefault(spec[0], []).append((count[0], pattern))
        count[0] += 1
        return (count[0] - 1, "found")

    return [one(s) for s in specs], wanted


_EPOCH = datetime.datetime(1970, 1, 1, tzinfo=datetime.timezone.utc)


def datetime_units(when, unit):
    """A ``datetime.datetime`` as the int64 ``cast_strings`` gives a timestamp of that instant in `unit` ("s" "ms" "us" "ns"):
    integer arithmetic on the timedelta since 1970-01-01T00:00:00Z, never a float; microseconds the unit has no digits for
    are cut (a floor), as the call cuts a fraction.  Aware, or naive, which means UTC."""
    if when.tzinfo is None or when.utcoffset() is None:
        when = when.replace(tzinfo=datetime.timezone.utc)
    delta = when - _EPOCH
    micros = (delta.days * 86400 + delta.seconds) * 10**6 + delta.microseconds
    per = _lib.CAST_UNIT_PER_SECOND[unit]
    return micros * (per // 10**6) if per >= 10**6 else micros // (10**6 // per)


def _cast_spec(spec):
    """"number", "timestamp" or ("timestamp", unit) -> (kind, unit)"""
    kind, unit = (spec, "ns") if isinstance(spec, str) else tuple(spec)
    if kind not in _lib.CAST_KINDS or unit not in _lib.CAST_UNITS:
        raise ValueError(f"a cast is 'number', 'timestamp' or ('timestamp', 's' | 'ms' | 'us' | 'ns') -- and 'string' for order / order_by only: {spec!r}")
    return kind, unit


def _cast(window, d_rows, d_select, rows, kind, unit, keep_numbers, what):
    """``cast_strings`` over `rows` records (int64[rows, 2]) -> (the cast records int64[rows, 2], the uint8[48] select result
    that goes with them).  Only the call's 48-byte result comes to the host."""
    w = window
    d_res, d_out, d_out_select = w.dev.cast_strings(w.d_window, w.length, _or_blank(d_rows, rows).contiguous(), d_select, kind, unit,
                                                    keep_numbers, capacity=rows, sync=False)
    code = _code(d_res)
    if code != 0:
        raise DocumentStreamError(code, f"window at {w.base}: {what} could not be cast")
    return d_out[:rows], d_out_select


def _bucket_numbers(width, origin, unit):
    """A bucket's width and origin as the two int64 ``bucket_rows`` takes.  width: an int, or a ``datetime.timedelta`` that is
    a whole number of `unit`; origin: an int, or a ``datetime.datetime`` (``datetime_units``).  unit: the unit of the column's
    timestamp cast, None without one -- then only ints will do."""
    def needs_unit(what, value):
        if unit is None:
            raise ValueError(f"a {what} needs its column cast to a timestamp: {value!r}")

    if isinstance(width, datetime.timedelta):
        needs_unit("timedelta width", width)
        micros = ((width.days * 86400 + width.seconds) * 10**6 + width.microseconds) * _lib.CAST_UNIT_PER_SECOND[unit]
        if micros % 10**6:
            raise ValueError(f"the width is no whole number of {unit!r}: {width!r}")
        width = micros // 10**6
    if isinstance(origin, datetime.datetime):
        needs_unit("datetime origin", origin)
        origin = datetime_units(origin, unit)
    if isinstance(width, bool) or isinstance(origin, bool) or not isinstance(width, int) or not isinstance(origin, int):
        raise ValueError(f"a width is an int or a timedelta, an origin an int or a datetime: {width!r}, {origin!r}")
    if not 1 <= width < 1 << 63 or not -(1 << 63) <= origin < 1 << 63:
        raise ValueError(f"a width lies in 1..2^63 - 1, an origin in int64: {width!r}, {origin!r}")
    return width, origin


def _bucket(window, d_rows, d_select, rows, width, origin, cast, what):
    """``bucket_rows`` over `rows` records (int64[rows, 2]), cast first where asked -> (the bucket records int64[rows, 2], the
    uint8[48] select result that goes with them).  Only 48-byte results come to the host."""
    w = window
    unit = None
    if cast is not None:
        kind, unit = _cast_spec(cast)
        d_rows, d_select = _cast(w, d_rows, d_select, rows, kind, unit, kind == "number", what)
        unit = unit if kind == "timestamp" else None
    width, origin = _bucket_numbers(width, origin, unit)
    d_res, d_out, d_out_select = w.dev.bucket_rows(_or_blank(d_rows, rows).contiguous(), d_select, width, origin, capacity=rows, sync=False)
    code = _code(d_res)
    if code != 0:
        raise DocumentStreamError(code, f"window at {w.base}: {what} could not be put into buckets")
    return d_out[:rows], d_out_select


def _cast_for_filter(window, d_fields, d_select, rows, specs, cast, index, what):
    """What ``where(..., cast=...)`` hands the filter: the columns the predicates name, copied, the cast ones replaced by
    their cast records (a quoted number next to a plain one is kept), and the specs re-numbered onto that copy with every
    ``datetime.datetime`` operand turned into its column's unit.  specs: already by column number.  -> (specs, d_fields)"""
    kinds = {index(name): _cast_spec(spec) for name, spec in cast.items()}

    def columns(spec):
        return columns(spec[1]) if len(spec) == 2 and spec[0] == "not" else {spec[0]}

    used = sorted(set().union(*[columns(s) for s in specs])) if specs else []
    place = {c: j for j, c in enumerate(used)}

    def one(spec):
        if len(spec) == 2 and spec[0] == "not":
            return ("not", one(spec[1]))
        c, rest = spec[0], list(spec[1:])
        if len(rest) == 2 and isinstance(rest[1], datetime.datetime):
            if kinds.get(c, ("", ""))[0] != "timestamp":
                raise ValueError(f"a datetime operand needs its column cast to a timestamp: {spec!r}")
            rest[1] = datetime_units(rest[1], kinds[c][1])
        return (place[c],) + tuple(rest)

    out = torch.zeros((max(len(used), 1), max(rows, 1), 2), dtype=torch.int64, device=d_fields.device)
    for c in used:
        if c in kinds and rows:
            kind, unit = kinds[c]
            out[place[c], :rows] = _cast(window, d_fields[c], d_select, rows, kind, unit, kind == "number", what)[0]
        elif rows:
            out[place[c], :rows] = d_fields[c, :rows]
    return [one(s) for s in specs], out


_TAGS = '{["ldtfn'  # the value tags of an msj_field


class DictionaryColumn:
    """A byte column in the dictionary layout ON THE DEVICE (``msj_dictionary_device``; ``Window.categories``,
    ``ListColumn.categories``, ``ElementFields.categories``, ``MapColumn.key_categories``).  codes int32[rows]: -1 for a row
    without a value, else the value's number in the order of first appearance; offsets int64[n_distinct + 1] and bytes
    uint8[total]: value c is bytes[offsets[c]:offsets[c + 1]]; first int32[n_distinct]: the row value c first appears in;
    valid bool[rows], the column's own validity."""

    def __init__(self, codes, offsets, data, first, valid, dev=None):
        self.codes, self.offsets, self.bytes, self.first, self.valid, self.dev = codes, offsets, data, first, valid, dev

    @property
    def n_distinct(self):
        return self.first.shape[0]

    def order(self, max_rounds=None):
        """The distinct values in byte order ON THE DEVICE (``msj_dictionary_order_device``) -> ``DictionaryOrder``: the
        entries ascending by value and every entry's rank, so that ``order().rank_records(self.codes)`` are records that
        sort, filter and aggregate like the strings.  max_rounds: the rounds of eight bytes one call compares (None: the
        call's default); values that agree further are ordered by repeating the call."""
        if self.dev is None:
            raise ValueError("this DictionaryColumn was made without a device")
        return _dictionary_order(self.dev, self.offsets, self.bytes, self.n_distinct, max_rounds, "the dictionary")

    def counts(self):
        """Rows per value, int64[n_distinct], on the device (``torch.bincount`` of the codes that are not -1)."""
        codes = self.codes[self.codes >= 0].to(torch.int64)
        return torch.bincount(codes, minlength=self.n_distinct)

    def values(self):
        """The distinct values as str in the order of first appearance: the dictionary comes to the host, the codes do not."""
        off, data = self.offsets.cpu().tolist(), self.bytes.cpu().numpy().tobytes()
        return [data[off[c]:off[c + 1]].decode("utf-8", "surrogateescape") for c in range(self.n_distinct)]

    def to_python(self):
        """(the distinct values as ``values`` gives them, the codes as a list)."""
        return self.values(), self.codes.cpu().tolist()


def _dictionary(window, column, what):
    """``dictionary`` over a column (offsets int64[rows + 1], bytes uint8[total], valid bool[rows]) as the column calls
    return it, sized from the call's own layout-only pass -> ``DictionaryColumn``"""
    offsets, data, valid = column
    rows = valid.shape[0]
    res, codes, d_off, d_first, d_bytes = window.dev.dictionary(offsets, data, _or_blank(valid.view(torch.uint8), rows), rows=rows)
    if res.code != 0:
        raise DocumentStreamError(int(res.code), f"window at {window.base}: the strings of {what} could not be dictionary-encoded")
    n = int(res.n_distinct)
    return DictionaryColumn(codes[:rows], d_off[:n + 1], d_bytes[:int(res.dict_bytes)], d_first[:n], valid, window.dev)


class DictionaryOrder:
    """A dictionary's entries in the byte order of their values ON THE DEVICE (``msj_dictionary_order_device``;
    ``DictionaryColumn.order``, ``RunningDictionary.order``).  sorted int32[n]: the entry numbers ascending by value -- unsigned
    bytes, a proper prefix first, which for UTF-8 is code-point order; no collation, no case folding --, equal values by
    entry number; rank int32[n]: per entry the number of smaller values, so for a real dictionary ``sorted[rank[c]] == c``;
    result: the last call's ``MsjDictionaryOrderResult``; d_result: the uint8[48] device tensor that holds it."""

    def __init__(self, dev, offsets, data, sorted_entries, rank, d_result, result):
        self.dev, self.offsets, self.bytes = dev, offsets, data
        self.sorted, self.rank, self.d_result, self.result = sorted_entries, rank, d_result, result

    @property
    def n_entries(self):
        return self.sorted.shape[0]

    def values(self):
        """The distinct values as str, ascending: the dictionary and the order come to the host."""
        off, data = self.offsets.cpu().tolist(), self.bytes.cpu().numpy().tobytes()
        return [data[off[c]:off[c + 1]].decode("utf-8", "surrogateescape") for c in self.sorted.cpu().tolist()]

    def rank_records(self, codes):
        """A column of this dictionary's codes (int32[rows]) as records that order like the strings
        (``msj_rank_rows_device``) -> (records int64[rows, 2], the uint8[48] select result that counts them): a row's value's
        rank as an int64 value, the record of a missing value for a row without one (-1, -2, a code of a later window).
        ``sort_rows``, ``filter_rows``, ``aggregate`` and ``take_rows`` take them.  Nothing comes to the host."""
        rows = codes.shape[0]
        _, d_fields, d_select = self.dev.rank_rows(_or_blank(codes, rows).contiguous(), _or_blank(self.rank, self.n_entries), self.d_result, rows=rows,
                                                   rank_capacity=self.n_entries, capacity=rows, sync=False)
        return d_fields[:rows], d_select


def _dictionary_order(dev, offsets, data, n, max_rounds, what):
    """``dictionary_order`` over the n entries of (offsets int64[n + 1], bytes), repeated with MSJ_ORDER_CONTINUE while
    entries are still tied -> ``DictionaryOrder``.  Each call's 48-byte result comes to the host."""
    d_sorted = d_rank = None
    depth, resume = 0, False
    while True:
        res, d_sorted, d_rank = dev.dictionary_order(offsets, _or_blank(data, data.shape[0]), n_entries=n, capacity=n, dict_bytes_capacity=data.shape[0],
                                                     depth=depth, max_rounds=int(max_rounds or 0), resume=resume, d_sorted=d_sorted, d_rank=d_rank,
                                                     sync=False)
        d_result = res
        res = _lib.MsjDictionaryOrderResult.from_buffer_copy(d_result.cpu().numpy().tobytes())
        if res.code != errors.CAPACITY or res.n_tied == 0 or res.depth <= depth:
            break
        depth, resume = int(res.depth), True
    if res.code != 0 or res.n_entries != n:
        raise DocumentStreamError(int(res.code), f"{what} could not be ordered")
    return DictionaryOrder(dev, offsets, data, d_sorted[:n], d_rank[:n], d_result, res)


class RunningDictionary:
    """The dictionary a stream carries from window to window ON THE DEVICE (``msj_dictionary_extend_device``): it owns the
    three dictionary tensors -- offsets int64[dict_capacity + 1], first int32[dict_capacity], bytes uint8[bytes_capacity] --
    and knows how many entries they hold.  ``win.categories("/status", dictionary=rd)`` encodes a window's column against
    it, so that a value has ONE code in every window: ``counts()`` add, ``stats(..., by=..., dictionary=rd)`` give records
    that merge by position.  The tensors grow when a window's new values do not fit; a ``DictionaryColumn`` handed out
    before keeps the tensors it was made over.  One column per RunningDictionary: values of two columns share codes only
    when that is wanted."""

    def __init__(self, dev, dict_capacity=1024, bytes_capacity=16384):
        self.dev = dev
        self._n = self._n_bytes = 0
        self._allocate(max(int(dict_capacity), 1), max(int(bytes_capacity), 1))

    def _allocate(self, dict_capacity, bytes_capacity):
        """New tensors of these capacities with the entries held so far copied over on the device"""
        device = self.dev.device
        offsets = torch.zeros(dict_capacity + 1, dtype=torch.int64, device=device)
        first = torch.zeros(dict_capacity, dtype=torch.int32, device=device)
        data = torch.zeros(bytes_capacity, dtype=torch.uint8, device=device)
        if self._n:
            offsets[:self._n + 1] = self.offsets[:self._n + 1]
            first[:self._n] = self.first[:self._n]
            data[:self._n_bytes] = self.bytes[:self._n_bytes]
        self.offsets, self.first, self.bytes = offsets, first, data

    @property
    def n_distinct(self):
        return self._n

    @property
    def dict_capacity(self):
        return self.first.shape[0]

    @property
    def bytes_capacity(self):
        return self.bytes.shape[0]

    def values(self):
        """The values as str in code order: the dictionary comes to the host."""
        off, data = self.offsets[:self._n + 1].cpu().tolist(), self.bytes[:self._n_bytes].cpu().numpy().tobytes()
        return [data[off[c]:off[c + 1]].decode("utf-8", "surrogateescape") for c in range(self._n)]

    def order(self, max_rounds=None):
        """The values held so far in byte order ON THE DEVICE -> ``DictionaryOrder`` (see ``DictionaryColumn.order``): ranks
        for the codes of every window encoded so far.  A value added later changes the ranks: order again."""
        return _dictionary_order(self.dev, self.offsets[:self._n + 1], self.bytes[:self._n_bytes], self._n, max_rounds, "the running dictionary")

    def encode(self, column, frozen=False, what="a column"):
        """A column (offsets int64[rows + 1], bytes uint8[total], valid bool[rows]) as the column calls return it, encoded
        against this dictionary -> ``DictionaryColumn``: codes int32[rows] in THIS dictionary's numbering; offsets and bytes
        are views of the running dictionary as it stands after the call; first holds -1 for the values that came from
        earlier windows, else the row of this column; so ``counts()`` has ``n_distinct`` entries of the running dictionary.
        New values are appended; where they do not fit (MSJ_CAPACITY from clipping) the tensors are grown -- at least
        doubled, at least to what the result names --, the prior part copied on the device and the call repeated with the
        same number of prior entries.  frozen=True: nothing is appended, a value the dictionary does not hold gets -2.  Any
        other code raises ``DocumentStreamError``.  The call's 64-byte result comes to the host."""
        offsets, data, valid = column
        rows = valid.shape[0]
        d_valid = _or_blank(valid.view(torch.uint8), rows)
        while True:
            res, codes, _, _, _ = self.dev.dictionary_extend(offsets, data, d_valid, self.offsets, self.first, self.bytes, n_prior=self._n,
                                                             rows=rows, frozen=frozen)
            need, need_bytes = int(res.n_distinct), int(res.dict_bytes)
            if res.code != errors.CAPACITY or (need <= self.dict_capacity and need_bytes <= self.bytes_capacity):
                break  # (not clipped: done, or one of the conditions under which nothing is written)
            self._allocate(max(need, 2 * self.dict_capacity) if need > self.dict_capacity else self.dict_capacity,
                           max(need_bytes, 2 * self.bytes_capacity) if need_bytes > self.bytes_capacity else self.bytes_capacity)
        if res.code != 0 or res.n_rows != rows or res.n_prior != self._n:
            raise DocumentStreamError(int(res.code), f"{what} could not be encoded against the running dictionary")
        prior, self._n, self._n_bytes = self._n, need, need_bytes
        first = torch.full((need,), -1, dtype=torch.int32, device=codes.device)
        first[prior:] = self.first[prior:need]
        return DictionaryColumn(codes[:rows], self.offsets[:need + 1], self.bytes[:need_bytes], first, valid, self.dev)


def _key_specs(keys):
    """The keys of ``group_by``: "/status" | (path, "string" | "number"[, {"nulls"}]) | (path, "bucket", width[, origin][,
    {"nulls"}]) -> [(path, kind, width, origin, null_is_group)]"""
    if not isinstance(keys, list):
        raise ValueError(f"the keys are a list: {keys!r}")
    out = []
    for key in keys:
        rest = list(key[1:]) if isinstance(key, tuple) else ["string"]
        path = key[0] if isinstance(key, tuple) else key
        nulls = bool(rest) and isinstance(rest[-1], (set, frozenset))
        if nulls and set(rest.pop()) != {"nulls"}:
            raise ValueError(f'the flags of a key are {{"nulls"}}: {key!r}')
        kind = rest[0] if rest else None
        if kind in ("string", "number") and len(rest) == 1:
            out.append((path, kind, None, None, nulls))
        elif kind == "bucket" and len(rest) in (2, 3):
            out.append((path, kind, rest[1], rest[2] if len(rest) == 3 else 0, nulls))
        else:
            raise ValueError(f'a key is a path, (path, "string" | "number") or (path, "bucket", width[, origin]), with {{"nulls"}} behind it '
                             f"where no value is a group of its own: {key!r}")
    if not 1 <= len(out) <= _lib.KEY_MAX_PARTS:
        raise ValueError(f"1 to {_lib.KEY_MAX_PARTS} keys: {len(out)}")
    return out


def _decode_number_part(part):
    """The eleven bytes of a NUMBER part -> the canonical value: an integer inside int64 as an ``int``, anything else the
    ``float``; None for a null part (group_keys_math.h: decode_number)"""
    if part[0] != 0:
        return None
    hi, lo = int.from_bytes(part[1:9], "big"), int.from_bytes(part[9:11], "big")
    d = struct.unpack("<d", struct.pack("<Q", hi ^ (1 << 63) if hi >> 63 else ~hi & ((1 << 64) - 1)))[0]
    if d.is_integer() and -(1 << 63) <= int(d) + lo < 1 << 63:
        return int(d) + lo
    return d


def _decode_keys(offsets, data, n, kinds, strings):
    """n keys of a key dictionary (host: offsets a list, data bytes) -> a list of tuples.  kinds: "string" | "number" per
    part; strings: per part the string dictionary's values, None for a number part"""
    out = []
    for g in range(n):
        key, at, row = data[offsets[g]:offsets[g + 1]], 0, []
        for kind, values in zip(kinds, strings):
            if kind == "number":
                row.append(_decode_number_part(key[at:at + 11]))
                at += 11
            else:
                code = int.from_bytes(key[at + 1:at + 5], "big")
                row.append(values[code] if key[at] == 0 and code < len(values) else None)
                at += 5
        out.append(tuple(row))
    return out


class GroupKeys(DictionaryColumn):
    """The groups of ``group_by`` ON THE DEVICE: a ``DictionaryColumn`` over the rows' composite byte keys
    (``msj_group_keys_device``, then ``msj_dictionary_device`` or a ``RunningGroups``' dictionary).  codes int32[rows]: the
    row's group in the order of first appearance, -1 for a row without a key (a part without a value that is no group of its
    own); first int32[n_distinct]: the row group g first appears in; offsets / bytes: the distinct keys, key_width bytes
    each -- per part a tag byte, then a number's order-preserving key or a string's code; kinds: "string" | "number" per
    part; parts: per part the string part's ``DictionaryColumn``, None for a number.  ``counts()`` as every dictionary
    column's.  ``order()``: the groups in key order -- the first key major, numbers as reals, a string part by its code (the
    order of first appearance; ``RunningDictionary.order`` has the byte order), no value last."""

    def __init__(self, column, key_width, kinds, parts):
        super().__init__(column.codes, column.offsets, column.bytes, column.first, column.valid, column.dev)
        self.key_width, self.kinds, self.parts = key_width, list(kinds), list(parts)

    def values(self):
        """The groups' keys as tuples, decoded FROM THE KEY BYTES on the host: a number part as an ``int`` (an integer inside
        int64: 200, 200.0 and 2e2 are the one group 200) or a ``float``, a string part as its dictionary's value, a part
        without a value as None.  The key dictionary and the string parts' dictionaries come to the host, the codes do not."""
        strings = [p.values() if p is not None else None for p in self.parts]
        return _decode_keys(self.offsets.cpu().tolist(), self.bytes.cpu().numpy().tobytes(), self.n_distinct, self.kinds, strings)


class RunningGroups:
    """The groups a stream carries from window to window ON THE DEVICE: one ``RunningDictionary`` per string part of `keys`
    and one for the composite keys.  ``win.group_by(keys, dictionary=rg)`` and ``win.stats(paths, by=keys, dictionary=rg)``
    encode each window against them, so that group g is the same key tuple in every window and the windows' records merge
    by position (include/msj_stage1.h, "Merging two windows' records").  keys: as ``group_by`` takes them, the same in every
    window."""

    def __init__(self, dev, keys, dict_capacity=1024):
        self.dev, self.specs = dev, _key_specs(keys)
        self.kinds = ["string" if s[1] == "string" else "number" for s in self.specs]
        self.strings = [RunningDictionary(dev, dict_capacity) if k == "string" else None for k in self.kinds]
        width = sum(5 if k == "string" else 11 for k in self.kinds)
        self.keys = RunningDictionary(dev, dict_capacity, dict_capacity * width)

    @property
    def n_distinct(self):
        return self.keys.n_distinct

    def values(self):
        """The key tuples in group order, as ``GroupKeys.values`` gives them: the dictionaries come to the host."""
        k = self.keys
        strings = [rd.values() if rd is not None else None for rd in self.strings]
        return _decode_keys(k.offsets[:k._n + 1].cpu().tolist(), k.bytes[:k._n_bytes].cpu().numpy().tobytes(), k._n, self.kinds, strings)

    def order(self, max_rounds=None):
        """The groups held so far in key order ON THE DEVICE -> ``DictionaryOrder`` (see ``GroupKeys``)."""
        return self.keys.order(max_rounds)


class GroupStats:
    """Count, sum, min and max per group ON THE DEVICE (``msj_aggregate_device``; ``Window.stats``, ``RowSelection.stats``,
    ``ElementFields.stats``, ``ListColumn.stats``).  keys: the ``DictionaryColumn`` of the grouping path, whose value g names
    group g -- for a list of keys the ``GroupKeys``, whose value g is a tuple -- (None: one group, or a group per row of a
    list column); pointers: the aggregated columns' names; records
    uint8[n_columns, n_groups, 48], the ``msj_aggregate`` records as the call wrote them, and as views of them: n_rows
    int64[n_groups]; n_values, sums, mins, maxs int64[n_columns, n_groups] -- sums, mins and maxs hold an int64 where
    sum_types / min_types / max_types (uint8, the same shape) say ord("l"), the pattern of a double where they say ord("d"),
    nothing where they say 0; flags uint8[n_columns, n_groups]: ``_lib.AGG_INT_OVERFLOW``, ``_lib.AGG_INFINITE``.  n_ungrouped,
    n_skipped: the result's counts.  Every bit is a pure function of the rows: the same from run to run, for every order."""

    def __init__(self, keys, pointers, records, result):
        self.keys, self.pointers, self.records = keys, list(pointers), records
        words = records.view(torch.int64).view(records.shape[0], records.shape[1], 6)
        self.n_rows, self.n_values = words[0, :, 0], words[:, :, 1]
        self.sums, self.mins, self.maxs = words[:, :, 2], words[:, :, 3], words[:, :, 4]
        self.sum_types, self.min_types, self.max_types, self.flags = (records[:, :, 40 + i] for i in range(4))
        self.n_ungrouped, self.n_skipped = int(result.n_ungrouped), int(result.n_skipped)

    @property
    def n_groups(self):
        return self.records.shape[1]

    def to_python(self):
        """A dict per group: "key" (the group's value; absent without keys) and per aggregated column its pointer with
        {"n_rows", "n_values", "sum", "min", "max", "flags"} -- an 'l' as a Python ``int``, a 'd' as a ``float``, None for a
        group without a number value.  The records and the dictionary come to the host."""
        rec = self.records.cpu().numpy()
        words = rec.view("<u8").reshape(rec.shape[0], rec.shape[1], 6)

        def number(tag, bits):
            bits = int(bits)
            if tag == ord("l"):
                return bits - (1 << 64) if bits >> 63 else bits
            return struct.unpack("<d", struct.pack("<Q", bits))[0] if tag == ord("d") else None

        keys = self.keys.values() if self.keys is not None else None
        out = []
        for g in range(rec.shape[1]):
            row = {} if keys is None else {"key": keys[g]}
            for c, pointer in enumerate(self.pointers):
                w, tags = words[c, g], rec[c, g, 40:44]
                row[pointer] = {"n_rows": int(w[0]), "n_values": int(w[1]), "sum": number(tags[0], w[2]), "min": number(tags[1], w[3]),
                                "max": number(tags[2], w[4]), "flags": int(tags[3])}
            out.append(row)
        return out


def _stats(window, d_fields, d_select, rows, columns, pointers, cast, keys, d_codes, n_groups, what):
    """``aggregate`` over the named columns of d_fields (int64[n_columns, rows, 2]), cast first where asked -> ``GroupStats``.
    columns: their numbers in d_fields; cast: {column number: spec}; d_codes: int32[rows] or None; the 48-byte result comes to
    the host."""
    w = window
    if not columns:
        raise ValueError("stats of no column")
    fields = torch.zeros((len(columns), max(rows, 1), 2), dtype=torch.int64, device=d_fields.device)
    for j, c in enumerate(columns):
        if not rows:
            break
        if c in cast:
            kind, unit = _cast_spec(cast[c])
            fields[j, :rows] = _cast(w, d_fields[c], d_select, rows, kind, unit, kind == "number", what)[0]
        else:
            fields[j, :rows] = d_fields[c, :rows]
    if d_codes is not None:
        d_codes = _or_blank(d_codes, rows).to(torch.int32).contiguous()
    res, d_groups = w.dev.aggregate(fields, d_select, d_codes, n_groups=n_groups, groups_capacity=max(n_groups, 1))
    if res.code != 0 or res.n_rows != rows:
        raise DocumentStreamError(int(res.code), f"window at {w.base}: {what} could not be aggregated")
    records = d_groups[:len(columns) * max(n_groups, 1) * 48].view(len(columns), max(n_groups, 1), 48)[:, :n_groups]
    return GroupStats(keys, pointers, records, res)


def _sort_keys(keys, index, descending=False):
    """A path or index, (path, "asc" | "desc"), or a list of them, major key first -> [(column number, descending)]"""
    def one(key):
        if isinstance(key, tuple):
            if len(key) != 2 or key[1] not in ("asc", "desc"):
                raise ValueError(f'a sort key is a path or (path, "asc" | "desc"): {key!r}')
            return index(key[0]), key[1] == "desc"
        return index(key), bool(descending)

    out = [one(k) for k in keys] if isinstance(keys, list) else [one(keys)]
    if not out:
        raise ValueError("an order by no key")
    return out


def _string_ranks(window, d_fields, d_select, rows, c, what):
    """The cast "string" of ``order`` / ``order_by``: column c's strings -> their dictionary -> its order -> the rows' rank
    records int64[rows, 2] (``msj_string_column_device``, ``msj_dictionary_device``, ``msj_dictionary_order_device``,
    ``msj_rank_rows_device``): numbers that ``sort_rows`` orders as the strings order in bytes.  A row without a string has no
    number value."""
    column = _string_column(window, d_fields, d_select, rows, c, None, f"column {c} of {what}")
    categories = _dictionary(window, column, f"column {c} of {what}")
    return categories.order().rank_records(categories.codes)[0]


def _order(window, d_fields, d_select, rows, keys, limit, values_only, cast, what):
    """``sort_rows`` over `rows` records per column of d_fields (int64[n_columns, rows, 2]), one call per key, the minor key
    first and each call's order the next one's d_rows_in (the sort is stable); the last call gets the limit and values_only.
    keys: [(column number, descending)], major first; cast: {column number: spec}.  -> (order int32[K], the uint8[48] select
    result that counts it).  A code of an earlier call reaches the last one through that select result: only the last
    call's 48-byte result comes to the host."""
    w = window
    if limit is not None and int(limit) <= 0:
        raise ValueError(f"limit is None or at least 1: {limit!r}")
    d_in = d_in_select = None
    for j, (c, descending) in enumerate(reversed(keys)):
        last = j == len(keys) - 1
        column = d_fields[c]
        if c in cast and rows and cast[c] == "string":
            column = _string_ranks(w, d_fields, d_select, rows, c, what)
        elif c in cast and rows:
            kind, unit = _cast_spec(cast[c])
            column = _cast(w, column, d_select, rows, kind, unit, kind == "number", what)[0]
        res, d_in, d_in_select = w.dev.sort_rows(_or_blank(column, rows).contiguous(), d_select, d_in, d_in_select, descending=descending,
                                                 values_only=values_only and last, limit=int(limit or 0) if last else 0, capacity=rows, sync=last)
    if res.code != 0 or res.n_rows != rows:
        raise DocumentStreamError(int(res.code), f"window at {w.base}: {what} could not be ordered")
    return d_in[:int(res.n_written)], d_in_select


def _rows_of_elements(offsets, n_elements):
    """The row of every element of a list column, int32[n_elements], from its offsets (torch)"""
    at = torch.arange(n_elements, dtype=torch.int64, device=offsets.device)
    return torch.searchsorted(offsets[1:].contiguous(), at, right=True).to(torch.int32)


class _Records:
    """Records by column over a window: what ``Window``, ``RowSelection`` and ``ElementFields`` are and, as ``_OneColumn``,
    what a ``ListColumn`` and the keys of a ``MapColumn`` run on.  A class says what its rows are through: window, the
    ``Window``; fields int64[n_columns, rows, 2], one ``msj_field`` per (column, row); d_select uint8[48], the device
    ``msj_select_documents_result`` that counts the rows; paths, whose ``index`` turns a pointer or an index into a column's
    number and whose ``pointers`` name the columns; _rows_are, the rows' name in messages; _parent, what ``elements`` and
    ``entries`` hand on as the new column's parent.

    The calls run on the window's arrays and on the records where they lie; of a call only its small result comes to the
    host.  A row is not valid, and empty, where the value is not of the kind asked for, the key is missing or the document
    has a verdict code.  Like every array a Window carries, the window's own arrays are reused by the next window: use what
    a method returns before the iterator advances."""

    _rows_are = "the rows"
    _parent = None

    @property
    def _window(self):
        return self.window

    @property
    def _records(self):
        return self.fields

    def _at(self, path_or_index):
        """(the window, the records, the rows, the column's number, the column's name in messages)"""
        fields = self._records
        p = self.paths.index(path_or_index)
        return self._window, fields, fields.shape[1], p, f"path {p} of {self._rows_are}"

    def column(self, path_or_index):
        """The records of one path as a numpy structured array (FIELD_DTYPE), one per row: one host copy."""
        _, fields, _, p, _ = self._at(path_or_index)
        return np.ascontiguousarray(fields[p].cpu().numpy()).view(FIELD_DTYPE).reshape(-1)

    def values(self, path_or_index):
        """The values of one path as a Python list, one per row: None where the record has a code (20 NO_SUCH_FIELD, 17
        INCORRECT_TYPE, an invalid document's), see ``field_value``.  The window's bytes, d_idx and d_end come to the host
        once per window."""
        col = self.column(path_or_index)
        host = self._window._host_arrays()
        return [field_value(r, *host) for r in col]

    def _number_column(self, path_or_index, dtype):
        """The numbers of one path as a column ON THE DEVICE, from the records alone (torch operations, no call), as the
        module's ``number_column`` gives them: (values dtype[rows], valid bool[rows])"""
        _, fields, _, p, _ = self._at(path_or_index)
        return number_column(fields[p], dtype)

    def _cast_column(self, path_or_index, kind, unit, keep_numbers):
        """``_cast`` over one path's records"""
        w, fields, rows, p, what = self._at(path_or_index)
        return _cast(w, fields[p], self.d_select, rows, kind, unit, keep_numbers, what)

    def timestamps(self, path_or_index, unit="ns"):
        """The RFC 3339 strings of one path -- "ts":"2024-05-01T12:34:56.789Z" -- as a column ON THE DEVICE
        (``msj_cast_strings_device``, then ``number_column``): (values int64[rows], valid bool[rows]), the count of `unit` ("s"
        "ms" "us" "ns") since 1970-01-01T00:00:00Z, offsets applied, a fraction cut to the unit.  Not valid, value 0: a string
        that is no timestamp (or, in "ns", one outside 1677-09-21 .. 2262-04-11), a value that is no string, a missing key, a
        document with a verdict code.  Only the call's 48-byte result comes to the host."""
        return number_column(self._cast_column(path_or_index, "timestamp", unit, False)[0], torch.int64)

    def parsed_numbers(self, path_or_index, dtype=torch.float64, keep_numbers=True):
        """The numbers of one path that are written as strings -- "price":"12.50", "id":"9007199254740993" -- as a column ON
        THE DEVICE: (values dtype[rows], valid bool[rows]) as ``number_column`` gives them, over the cast records: an integer
        stays an exact int64.  keep_numbers: a value that already is a number counts as well."""
        return number_column(self._cast_column(path_or_index, "number", "ns", keep_numbers)[0], dtype)

    def strings(self, path_or_index, bytes_capacity=None):
        """The string values of one path as a column ON THE DEVICE (``msj_string_column_device``): (offsets int64[rows + 1],
        bytes uint8[total], valid bool[rows]) -- row k's unescaped UTF-8 is bytes[offsets[k]:offsets[k + 1]], empty where
        valid[k] is False (the value is no string, the key is missing, the document has a verdict code).  The byte buffer
        starts from a guess (bytes_capacity: the caller's) and, when the call says it was too small, is made as large as the
        call asks and the call runs once more."""
        w, fields, rows, p, what = self._at(path_or_index)
        return _string_column(w, fields, self.d_select, rows, p, bytes_capacity, what)

    def categories(self, path_or_index, bytes_capacity=None, dictionary=None, frozen=False):
        """The string values of one path in the dictionary layout ON THE DEVICE (``msj_dictionary_device`` over
        ``strings(path)``) -> ``DictionaryColumn``: codes int32[rows], -1 where the row has no string, else the value's
        number in the order of first appearance, and the distinct values once.  A low-cardinality column -- a status, a
        country, a device id -- is grouped, compared and counted (``counts()``) without moving a byte to the host.
        dictionary: a ``RunningDictionary``, against which the column is encoded instead (``RunningDictionary.encode``): a
        value has the same code in every window.  frozen=True: nothing is added to it, a value it does not hold is -2."""
        column = self.strings(path_or_index, bytes_capacity)
        what = self._at(path_or_index)[-1]
        if dictionary is not None:
            return dictionary.encode(column, frozen=frozen, what=f"window at {self._window.base}: the strings of {what}")
        if frozen:
            raise ValueError("frozen=True needs a dictionary")
        return _dictionary(self._window, column, what)

    def raw(self, path_or_index, compact=False, bytes_capacity=None):
        """The JSON text of one path's values as a column ON THE DEVICE (``msj_raw_column_device``): (offsets int64[rows + 1],
        bytes uint8[total], valid bool[rows]) -- row k's text is bytes[offsets[k]:offsets[k + 1]], the source's own bytes from
        the value's first to its last, whatever the value is: the way to a container's text without the window on the host.
        "" is the whole document, or the whole element.  Empty where valid[k] is False (the key is missing, the document has
        a verdict code).  compact: the blanks between tokens dropped, so that a pretty-printed window gives the bytes of its
        minified twin: ``raw("", compact=True)`` over documents is those documents as minified NDJSON lines.  The byte buffer
        starts from a guess (bytes_capacity: the caller's) and is grown once, as in ``strings``."""
        w, fields, rows, p, what = self._at(path_or_index)
        return _raw_column(w, fields[p], self.d_select, rows, compact, bytes_capacity, what)

    def match(self, path_or_index, patterns, raw=False, compact=False):
        """Substring patterns over the string values of one path ON THE DEVICE (``msj_match_strings_device`` over
        ``strings(path)``) -> (fields int64[n_patterns, rows, 2], the uint8[48] ``msj_select_documents_result`` that goes with
        them): per (pattern, row) the 'l' record of the first place where the pattern matches the unescaped value, or the
        record of a missing value -- no match, no string, a missing key, a document with a verdict code.  patterns: 1 to 16
        specs as ``Stage1Device.compile_patterns`` takes them: ``b"timeout"`` (contains), ``([b"GET ", b".png"], {"at_start",
        "at_end", "nocase"})``.  raw=True: over ``raw(path, compact)``, the values' JSON text, instead: ``win.match("",
        [b"timeout"], raw=True)`` is grep over the window's lines.  ``filter_rows``, ``take_rows``, ``aggregate`` and
        ``sort_rows`` take the records as they take a select call's.  Only 48-byte results come to the host."""
        w, _, rows, _, what = self._at(path_or_index)
        d_off, d_bytes, valid = self.raw(path_or_index, compact) if raw else self.strings(path_or_index)
        compiled = w.dev.compile_patterns(patterns)
        try:
            d_res, d_fields, d_sel = w.dev.match_strings(compiled, d_off, valid.view(torch.uint8), d_bytes, rows=rows, sync=False)
        finally:  # (the patterns live for the call, as ``_filter``'s predicates do: freeing their device memory waits for the
            compiled.close()  # device, so the kernels that were just enqueued have read them)
            w.dev._paths.remove(compiled)
        code = _code(d_res)
        if code != 0:
            raise DocumentStreamError(code, f"window at {w.base}: {what} could not be matched")
        return d_fields[:, :rows], d_sel

    def elements(self, path_or_index, elements_capacity=None):
        """The arrays of one path as a list column -- ``tags``, ``items[*].tags`` -- ON THE DEVICE
        (``msj_array_elements_device``) -> ``ListColumn`` with one row per row of these records: offsets int64[rows + 1], one
        ``msj_field`` per element back to back, valid bool[rows]; a missing key and a value that is no array are rows that are
        not valid.  The element buffer starts from a guess (elements_capacity: the caller's) and, when the call says it was
        too small, is made as large as the call asks and the call runs once more."""
        w, fields, rows, p, what = self._at(path_or_index)
        return _array_elements(w, fields[p], self.d_select, rows, elements_capacity, self._parent, what)

    def entries(self, path_or_index, entries_capacity=None):
        """The objects of one path as a map column -- "attrs":{"color":"red",...} with the keys as data, ``items[*].dims`` --
        ON THE DEVICE (``msj_object_entries_device``) -> ``MapColumn`` with one row per row of these records: offsets
        int64[rows + 1], a key and a value ``msj_field`` per entry back to back, valid bool[rows]; a missing key and a value
        that is no object are rows that are not valid.  The buffers start from a guess (entries_capacity: the caller's) and
        are grown once, as in ``elements``."""
        w, fields, rows, p, what = self._at(path_or_index)
        return _object_entries(w, fields[p], self.d_select, rows, entries_capacity, self._parent, what)

    def stats(self, paths, by=None, cast=None, dictionary=None, frozen=False):
        """Count, sum, min and max of paths per group ON THE DEVICE (``msj_aggregate_device``) -> ``GroupStats``:
        ``win.stats(["/latency_ms"], by="/status")`` is how many lines, what total, smallest and largest latency per status.
        by: a path whose strings are dictionary-encoded first (``categories``): group g is the g-th distinct value, a row
        without a string is in no group; None: all rows are one group; a LIST of keys as ``group_by`` takes them --
        ``by=["/status", ("/ts", "bucket", timedelta(minutes=1))]`` with ``cast={"/ts": ("timestamp", "ms")}`` is errors per
        minute per status --: ``keys`` is then the ``GroupKeys``, "key" a tuple, and `dictionary` a ``RunningGroups``.  An int64 stays an int64 -- the sum of integers is
        the exact integer while it fits -- and a sum with doubles is rounded once: the same bits from run to run and for every
        order of the lines.  cast: ``{"/ts": ("timestamp", "ms"), "/price": "number"}`` as in ``where``, so that a timestamp
        has a minimum and a maximum and a quoted number a sum.  The call's 48-byte result comes to the host.
        dictionary: a ``RunningDictionary`` for `by` (``categories``): the groups are then ITS values, n_groups its
        n_distinct after this window, so that record g is the same value in every window and the windows' records merge
        by position (include/msj_stage1.h, "Merging two windows' records"); frozen=True as in ``categories``."""
        return self._grouped(paths, by, cast, dictionary=dictionary, frozen=frozen)

    def bucket(self, path_or_index, width, origin=0, cast=None):
        """One path's numbers floored to multiples of a width ON THE DEVICE (``msj_bucket_rows_device``) -> (records
        int64[rows, 2], the uint8[48] ``msj_select_documents_result`` that goes with them), as ``Window.cast`` returns its
        records: ``origin + floor((floor(v) - origin) / width) * width`` as an exact int64, a floor also below the origin.
        cast: "number", "timestamp" or ("timestamp", unit), applied first as in ``where``: ``win.bucket("/ts",
        datetime.timedelta(minutes=1), cast=("timestamp", "ms"))`` is every line's minute.  width: an int of at least 1, or a
        ``timedelta`` that is a whole number of the cast's unit; origin: an int, or a ``datetime`` in the cast's unit.  A
        value that is no number becomes code 17, a bucket outside int64 code 9.  Only 48-byte results come to the host."""
        w, fields, rows, p, what = self._at(path_or_index)
        return _bucket(w, fields[p], self.d_select, rows, width, origin, cast, what)

    def group_by(self, keys, cast=None, dictionary=None, frozen=False):
        """The rows grouped by 1 to 8 keys at once ON THE DEVICE (``msj_group_keys_device``, then ``msj_dictionary_device``)
        -> ``GroupKeys``.  keys, a list, the major key first: ``"/status"`` -- a string part: the path's ``categories`` codes;
        ``("/status", "string", {"nulls"})`` -- the same, and a row without a string is a group of its own instead of being in
        none; ``("/code", "number")`` -- the numbers as reals: 200, 200.0 and 2e2 are one group; ``("/ts", "bucket", width[,
        origin])`` -- ``bucket``'s numbers.  cast: ``{"/ts": ("timestamp", "ms")}``, applied first as in ``where``.
        dictionary: a ``RunningGroups`` made for the same keys: the groups are then ITS groups, the same in every window;
        frozen=True: nothing is added to it, a row whose key it does not hold is -2 (a string it does not hold is a part
        without a value).  Only 48- and 64-byte results come to the host.  Out of scope: calendar months and time zones, more than 8 keys, keys on raw JSON text (``raw`` +
        ``categories`` serve those)."""
        w, fields, index = self._window, self._records, self.paths.index
        rows = fields.shape[1]
        specs = _key_specs(keys)
        if dictionary is not None and (not isinstance(dictionary, RunningGroups) or dictionary.specs != specs):
            raise ValueError("the dictionary of a list of keys is a RunningGroups made for the same keys")
        if frozen and dictionary is None:
            raise ValueError("frozen=True needs a dictionary")
        casts = {index(k): v for k, v in (cast or {}).items()}
        tensors, kinds, parts = [], [], []
        for j, (path, kind, width, origin, nulls) in enumerate(specs):
            c = index(path)
            what = f"path {c} of {self._rows_are}"
            if kind == "string":
                column = self.categories(path, dictionary=dictionary.strings[j] if dictionary is not None else None, frozen=frozen)
                tensors.append((_or_blank(column.codes, rows).contiguous(), nulls))
                parts.append(column)
            elif kind == "bucket":
                tensors.append((_or_blank(_bucket(w, fields[c], self.d_select, rows, width, origin, casts.get(c), what)[0], rows).contiguous(), nulls))
                parts.append(None)
            else:
                records = fields[c]
                if c in casts:
                    k, unit = _cast_spec(casts[c])
                    records = _cast(w, records, self.d_select, rows, k, unit, k == "number", what)[0]
                tensors.append((_or_blank(records, rows).contiguous(), nulls))
                parts.append(None)
            kinds.append("string" if kind == "string" else "number")
        d_res, d_off, d_valid, d_bytes = w.dev.group_keys(tensors, self.d_select, capacity=rows, sync=False)
        code = _code(d_res)
        if code != 0:
            raise DocumentStreamError(code, f"window at {w.base}: the keys of {self._rows_are} could not be laid out")
        width = sum(_lib.KEY_PART_BYTES[_lib.KEY_CODE if k == "string" else _lib.KEY_NUMBER] for k in kinds)
        column = (d_off[:rows + 1], d_bytes[:rows * width], d_valid[:rows].view(torch.bool))
        what = f"the keys of {self._rows_are}"
        if dictionary is not None:
            encoded = dictionary.keys.encode(column, frozen=frozen, what=f"window at {w.base}: {what}")
        else:
            encoded = _dictionary(w, column, what)
        return GroupKeys(encoded, width, kinds, parts)

    def _grouped(self, paths, by, cast, d_list_offsets=None, dictionary=None, frozen=False):
        """``stats``; d_list_offsets: a list column's offsets over these rows, for a group per row of it -- the element's
        row number, computed from the offsets with torch, being its code"""
        w, fields, index = self._window, self._records, self.paths.index
        rows = fields.shape[1]
        columns = [index(p) for p in paths]
        if by is None and (dictionary is not None or frozen):
            raise ValueError("a dictionary groups the rows of `by`")
        if isinstance(by, list):
            keys = self.group_by(by, cast=cast, dictionary=dictionary, frozen=frozen)
        else:
            keys = self.categories(by, dictionary=dictionary, frozen=frozen) if by is not None else None
        if keys is not None:
            d_codes, n_groups = keys.codes, keys.n_distinct
        elif d_list_offsets is not None:
            d_codes, n_groups = _rows_of_elements(d_list_offsets, rows), d_list_offsets.shape[0] - 1
        else:
            d_codes, n_groups = None, 1
        return _stats(w, fields, self.d_select, rows, columns, [self.paths.pointers[c] for c in columns],
                      {index(k): v for k, v in (cast or {}).items()}, keys, d_codes, n_groups, self._rows_are)

    def _filtered(self, specs, any, cast, d_list_offsets=None):
        """``where``'s filter: specs with the columns named by pointer or index, the cast columns cast for the predicates to
        see -> what ``_filter`` returns"""
        w, fields, index = self._window, self._records, self.paths.index
        rows = fields.shape[1]
        specs, seen = _column_specs(specs, index), fields
        specs, wanted = _match_specs(specs, fields.shape[0])
        if wanted:  # a column's strings, one call with all of its patterns, the match records as further columns
            found = {}
            for c, news in wanted.items():
                records = self.match(c, [pattern for _, pattern in news])[0]
                found.update({new: records[j:j + 1] for j, (new, _) in enumerate(news)})
            seen = torch.cat([fields[:, :rows]] + [found[new] for new in sorted(found)])
        if cast or wanted:
            specs, seen = _cast_for_filter(w, seen, self.d_select, rows, specs, cast or {}, index, self._rows_are)
            if wanted and seen.shape[0] > _lib.MAX_COLUMNS:
                raise ValueError(f"predicates on more than {_lib.MAX_COLUMNS} columns, the substring operators' included")
        return _filter(w, seen, self.d_select, rows, specs, any, self._rows_are, d_list_offsets)

    def _taken(self, d_take, d_take_select, n_take):
        """``_take`` of these records by n_take row numbers"""
        return _take(self._window, self._records, self.d_select, d_take, d_take_select, n_take, self._rows_are)

    def order(self, keys, limit=None, cast=None, values_only=False, descending=False):
        """The row numbers in the exact numeric order of one or more paths ON THE DEVICE (``msj_sort_rows_device``) ->
        (order int32[K], the uint8[48] ``msj_select_documents_result`` that counts it): what ``take_rows`` takes as d_take
        and d_take_select.  keys: a path or index, (path, "desc"), or a list of them, the major key first; descending: the
        direction of the keys that name none.  An int64 is compared with a double as real numbers -- 9007199254740993 lies
        between 9007199254740992.0 and 9007199254740994.0 --, equal values keep their order, rows without a number value
        come last (values_only: are left out).  limit: only the first so many.  cast: ``{"/ts": ("timestamp", "ns")}`` as
        in ``where``, so that ``order("/ts", cast={"/ts": ("timestamp", "ns")})`` is time order; and here alone "string":
        ``order("/name", cast={"/name": "string"})`` orders by the strings' bytes (code-point order for UTF-8, no collation)
        through the column's dictionary, its order and the rows' ranks (``msj_dictionary_order_device``,
        ``msj_rank_rows_device``), rows without a string last.  Only small results come to the host."""
        fields, index = self._records, self.paths.index
        return _order(self._window, fields, self.d_select, fields.shape[1], _sort_keys(keys, index, descending), limit, values_only,
                      {index(k): v for k, v in (cast or {}).items()}, self._rows_are)


class _Unnamed:
    """The paths of one column without a name: column 0, pointer "" """
    pointers = [""]
    index = staticmethod(range(1).__getitem__)


class _OneColumn(_Records):
    """One unnamed column of records int64[rows, 2] as a record view: the elements of a ``ListColumn``, the keys of a
    ``MapColumn``"""
    paths = _Unnamed

    def __init__(self, window, fields, d_select, rows_are, parent=None):
        self.window, self.fields, self.d_select, self._rows_are, self._parent = window, fields.unsqueeze(0), d_select, rows_are, parent


class MapColumn:
    """Objects as a map column ON THE DEVICE (``Window.entries``, ``ListColumn.entries``, ``ElementFields.entries``): the
    members of objects whose keys are data.  offsets int64[rows + 1]; key_fields and value_fields int64[n_entries, 2], one
    ``msj_field`` per entry back to back at the same position -- row k's entries are [offsets[k]:offsets[k + 1]], duplicate
    keys all kept in document order; valid bool[rows], False where the value is no object, the key is missing or the document
    has a verdict code (the row is empty then); d_keys_select / d_values_select uint8[48], the
    ``msj_select_documents_result`` of the key and of the value records; parent, the column whose records are this column's
    rows -- None for ``Window.entries``, whose rows are the documents.  Like every array a Window carries, the window's own
    arrays are reused by the next window: use the column before the iterator advances."""

    def __init__(self, window, offsets, valid, key_fields, value_fields, d_keys_select, d_values_select, parent=None):
        self.window, self.offsets, self.valid, self.parent = window, offsets, valid, parent
        self.key_fields, self.value_fields = key_fields, value_fields
        self.d_keys_select, self.d_values_select = d_keys_select, d_values_select

    @property
    def n_entries(self):
        return self.key_fields.shape[0]

    @property
    def _keys(self):
        return _OneColumn(self.window, self.key_fields, self.d_keys_select, "the keys of the entries")

    def keys(self, bytes_capacity=None):
        """The keys, unescaped, as a string column on the device (``msj_string_column_device`` over the key records):
        (offsets int64[n_entries + 1], bytes uint8[total], valid bool[n_entries])."""
        return self._keys.strings(0, bytes_capacity)

    def key_categories(self, bytes_capacity=None, dictionary=None, frozen=False):
        """The keys in the dictionary layout ON THE DEVICE (``msj_dictionary_device`` over ``keys()``) ->
        ``DictionaryColumn`` with one code per entry: the same few names repeated millions of times become one int32 each
        and the names once.  dictionary, frozen: a ``RunningDictionary`` to encode against, as in ``Window.categories``."""
        return self._keys.categories(0, bytes_capacity, dictionary=dictionary, frozen=frozen)

    def schema(self):
        """Which keys these objects have: for each distinct key in the order of first appearance (the key, how many entries
        carry it, the set of value tags -- ``{ [ " l d t f n`` -- seen under it).  Computed on the device: the key codes
        of ``key_categories``, the type byte of ``value_fields`` and ``torch.bincount``; only the distinct keys and one
        small table come to the host.  ``Window.entries("").schema()`` is therefore "which fields do these documents have
        at all" -- what a user has to know before writing ``select=[...]``."""
        cats = self.key_categories()
        keys, n = cats.values(), cats.n_distinct
        if n == 0:
            return []
        meta = self.value_fields[:, 1]
        tag, code = (meta >> 32) & 0xFF, (meta >> 48) & 0xFFFF
        kind = torch.full((256,), len(_TAGS), dtype=torch.int64, device=meta.device)
        kind[torch.tensor([ord(c) for c in _TAGS], device=meta.device)] = torch.arange(len(_TAGS), device=meta.device)
        width = len(_TAGS) + 1  # (the last column: a value record with a code, or a tag that is none)
        column = torch.where(code == 0, kind[tag], torch.full_like(tag, len(_TAGS)))
        codes = cats.codes.to(torch.int64)
        has = codes >= 0
        table = torch.bincount(codes[has] * width + column[has], minlength=n * width).view(n, width).cpu().tolist()
        return [(keys[c], sum(table[c]), {t for t, seen in zip(_TAGS, table[c]) if seen}) for c in range(n)]

    def values(self):
        """The values as a ``ListColumn`` that shares this column's offsets and validity: ``.numbers()``, ``.strings()``,
        ``.select()``, ``.elements()`` and ``.entries()`` (a map of maps) run on them."""
        return ListColumn(self.window, self.offsets, self.value_fields, self.valid, self.d_values_select, self)

    def to_python(self):
        """A dict per row, None where the row is no object; the first of duplicate keys wins, as in a selected container.
        The records come to the host, and the window's bytes, d_idx and d_end once per window."""
        w = self.window
        off, ok = self.offsets.cpu().tolist(), self.valid.cpu().tolist()
        host = w._host_arrays()
        as_records = lambda t: np.ascontiguousarray(t.cpu().numpy()).view(FIELD_DTYPE).reshape(-1)
        keys, values = as_records(self.key_fields), as_records(self.value_fields)
        pairs = lambda k: ((field_value(keys[j], *host), field_value(values[j], *host)) for j in range(off[k], off[k + 1]))
        return [_first_wins(pairs(k)) if ok[k] else None for k in range(len(ok))]


class ListColumn:
    """Arrays as a list column ON THE DEVICE (``Window.elements``, ``ListColumn.elements``, ``ElementFields.elements``,
    ``MapColumn.values``).
    offsets int64[rows + 1]; fields int64[n_elements, 2], one ``msj_field`` per element back to back -- row k's elements are
    fields[offsets[k]:offsets[k + 1]]; valid bool[rows], False where the value is no array, the key is missing or the
    document has a verdict code (the row is empty then); d_select uint8[48], the ``msj_select_documents_result`` of the
    element records; parent, the ``ListColumn`` or ``ElementFields`` whose records are this column's rows -- None for
    ``Window.elements``, whose rows are the documents.  The methods that ``Window`` has by path run here on the elements, the
    one column there is, and mean the same: see ``Window``'s.  Like every array a Window carries, the window's own arrays are
    reused by the next window: use the column before the iterator advances."""

    def __init__(self, window, offsets, fields, valid, d_select, parent=None):
        self.window, self.offsets, self.fields, self.valid, self.d_select = window, offsets, fields, valid, d_select
        self.parent = parent

    @property
    def n_elements(self):
        return self.fields.shape[0]

    @property
    def _one(self):
        return _OneColumn(self.window, self.fields, self.d_select, "the elements", self)

    def numbers(self, dtype=torch.float64):
        """The elements that are numbers, as ``number_column`` gives them: (values dtype[n_elements], valid
        bool[n_elements])."""
        return self._one._number_column(0, dtype)

    def timestamps(self, unit="ns"):
        """The elements that are RFC 3339 strings as int64 counts of `unit` since 1970-01-01T00:00:00Z ON THE DEVICE: (values
        int64[n_elements], valid bool[n_elements])."""
        return self._one.timestamps(0, unit)

    def parsed_numbers(self, dtype=torch.float64, keep_numbers=True):
        """The elements that are numbers written as strings: (values dtype[n_elements], valid bool[n_elements])."""
        return self._one.parsed_numbers(0, dtype, keep_numbers)

    def strings(self, bytes_capacity=None):
        """The elements that are strings as a column on the device: (offsets int64[n_elements + 1], bytes uint8[total],
        valid bool[n_elements])."""
        return self._one.strings(0, bytes_capacity)

    def categories(self, bytes_capacity=None, dictionary=None, frozen=False):
        """The elements that are strings in the dictionary layout ON THE DEVICE -> ``DictionaryColumn`` with one code per
        element, -1 where the element is no string.  dictionary, frozen: a ``RunningDictionary`` to encode against, as in
        ``Window.categories``."""
        return self._one.categories(0, bytes_capacity, dictionary=dictionary, frozen=frozen)

    def raw(self, compact=False, bytes_capacity=None):
        """The JSON text of every element as a column on the device: (offsets int64[n_elements + 1], bytes uint8[total],
        valid bool[n_elements]) -- a container's text too, without the window on the host.  compact: the blanks between
        tokens dropped."""
        return self._one.raw(0, compact, bytes_capacity)

    def elements(self, elements_capacity=None):
        """The arrays among this column's elements as a list column of their own -- a list of lists -- ON THE DEVICE ->
        ``ListColumn`` with one row per element of this column, aligned with this column's offsets; an element that is no
        array is a row that is not valid."""
        return self._one.elements(0, elements_capacity)

    def entries(self, entries_capacity=None):
        """The objects among this column's elements as a map column -- a list of maps, or the values of a ``MapColumn`` (a map
        of maps) -- ON THE DEVICE -> ``MapColumn`` with one row per element of this column; an element that is no object is a
        row that is not valid."""
        return self._one.entries(0, entries_capacity)

    def bucket(self, width, origin=0, cast=None):
        """The elements that are numbers floored to multiples of a width ON THE DEVICE -> (records int64[n_elements, 2], their
        select result), as every record view's ``bucket``."""
        return self._one.bucket(0, width, origin, cast)

    def order(self, descending=False, limit=None, cast=None, values_only=False):
        """The element numbers in the order of the elements' values ON THE DEVICE -> (order int32[K], its select result), as
        ``Window.order`` gives them; cast: "string" for elements that are strings, or a cast as in ``stats``."""
        return self._one.order(0, limit, {0: cast} if cast else None, values_only, descending)

    def stats(self, per_row=False, cast=None):
        """Count, sum, min and max of the elements that are numbers ON THE DEVICE (``msj_aggregate_device``) ->
        ``GroupStats`` with one column, "": over all elements as one group, or with per_row=True a group per row of this
        column -- ``sum(scores[*])`` per document -- the element's row number, computed from the offsets with torch, being
        its code.  cast: "number", "timestamp" or ("timestamp", unit) for elements that are strings, see ``Window.where``."""
        return self._one._grouped([0], None, {0: cast} if cast else None, self.offsets if per_row else None)

    def to_python(self):
        """A list per row, None where the row is no array; the elements as ``field_value`` gives them.  The element records
        come to the host, and the window's bytes, d_idx and d_end once per window."""
        w = self.window
        off, ok = self.offsets.cpu().tolist(), self.valid.cpu().tolist()
        recs = np.ascontiguousarray(self.fields.cpu().numpy()).view(FIELD_DTYPE).reshape(-1)
        host = w._host_arrays()
        return [[field_value(r, *host) for r in recs[off[k]:off[k + 1]]] if ok[k] else None for k in range(len(ok))]

    def select(self, pointers_or_paths):
        """Fields by path inside the elements -- ``items[*].sku`` -- ON THE DEVICE (``msj_select_elements_device``) ->
        ``ElementFields``: one ``msj_field`` per (path, element), each path a column aligned with this column's offsets.
        pointers_or_paths: JSON pointers (object keys only, "" the element itself) or what ``compile_paths`` made of them.
        The call runs on the window's arrays and the element records where they lie; only its 48-byte result comes to the
        host."""
        w, n = self.window, self.n_elements
        paths = pointers_or_paths if hasattr(pointers_or_paths, "handle") else w.dev.compile_paths(list(pointers_or_paths))
        res, d_fields = w.dev.select_elements(paths, w.d_window, w.length, *w._token_arrays(), _or_blank(self.fields, n), self.d_select,
                                              **w._number_records(), capacity=n, sync=False)
        code = _code(res)
        if code != 0:
            raise DocumentStreamError(code, f"window at {w.base}: the fields of the elements could not be selected")
        return ElementFields(self, paths, d_fields[:, :n], res)

    def _kept_elements(self, kept, d_kept_select, d_offsets):
        """What a filter over one record (or more, path-major) per element kept, as a list column: the element records taken,
        the offsets the re-based ones -> ``ListColumn`` with this column's rows and validity"""
        fields, d_esel = self._one._taken(kept, d_kept_select, kept.shape[0])
        return ListColumn(self.window, d_offsets, fields[0], self.valid, d_esel, self.parent)

    def where(self, specs, any=False, cast=None):
        """The elements that pass predicates -- ``tags[*] == "red"``, ``scores[*] > 0.5`` -- ON THE DEVICE
        (``msj_filter_rows_device`` with the list offsets re-based, ``msj_take_rows_device``) -> a ``ListColumn`` with this
        column's rows and validity, new offsets, and the records of the kept elements in their order.  specs: as for
        ``Stage1Device.compile_predicates``, the elements themselves being column 0.  cast: ``{0: ("timestamp", "ms")}`` or
        ``{0: "number"}``, see ``Window.where``; the records kept are the originals."""
        _, kept, d_kept_select, d_offsets = self._one._filtered(specs, any, cast, self.offsets)
        return self._kept_elements(kept, d_kept_select, d_offsets)


class ElementFields(_Records):
    """Fields by path inside the elements of a ``ListColumn`` ON THE DEVICE (``ListColumn.select``): the rows are the
    elements.  fields int64[n_paths, n_elements, 2], one ``msj_field`` per (path, element): element j of row k of the list
    column is fields[p, offsets[k] + j], so every path is a column of a list of structs -- ``items[*].at``,
    ``items[*].price``.  d_select uint8[48], the call's ``msj_select_documents_result``; paths, the compiled paths;
    list_column, the list column the rows came from.  The methods mean what they mean on ``Window``, over the elements."""

    _rows_are = "the elements"

    def __init__(self, column, paths, fields, d_select):
        self.list_column, self.paths, self.fields, self.d_select = column, paths, fields, d_select

    @property
    def n_elements(self):
        return self.fields.shape[1]

    @property
    def _window(self):
        return self.list_column.window

    @property
    def _parent(self):
        return self

    def numbers(self, path_or_index, dtype=torch.float64):
        """The numbers of one path as ``number_column`` gives them: (values dtype[n_elements], valid bool[n_elements])."""
        return self._number_column(path_or_index, dtype)

    def stats(self, paths, by=None, cast=None, per_row=False, dictionary=None, frozen=False):
        """Count, sum, min and max of paths of the elements ON THE DEVICE (``msj_aggregate_device``) -> ``GroupStats``, see
        ``Window.stats``.  by: a path whose strings group the elements; per_row=True instead: a group per row of the list
        column -- ``sum(items[*].qty)`` per document -- the element's row number, computed from the offsets with torch,
        being its code.  dictionary, frozen: a ``RunningDictionary`` for `by`, as in ``Window.stats``."""
        if by is not None and per_row:
            raise ValueError("by and per_row exclude each other")
        return self._grouped(paths, by, cast, self.list_column.offsets if per_row else None, dictionary=dictionary, frozen=frozen)

    def where(self, specs, any=False, cast=None):
        """The elements whose fields pass predicates -- ``items[*].qty > 1`` -- ON THE DEVICE (``msj_filter_rows_device`` with
        the list offsets re-based, ``msj_take_rows_device``) -> ``ElementFields`` over the kept elements, whose ``list_column``
        is a new ``ListColumn`` with the parent's rows and validity, the re-based offsets and the element records taken with
        the same vector: ``items[*]`` stays a list column.  specs: as for ``Stage1Device.compile_predicates``, the columns
        named by pointer or index.  cast: ``{"/at": ("timestamp", "ms"), "/price": "number"}``, see ``Window.where``; the
        records kept are the originals."""
        _, kept, d_kept_select, d_offsets = self._filtered(specs, any, cast, self.list_column.offsets)
        column = self.list_column._kept_elements(kept, d_kept_select, d_offsets)
        fields, d_fsel = self._taken(kept, d_kept_select, kept.shape[0])
        return ElementFields(column, self.paths, fields, d_fsel)

    def to_python(self):
        """A list per row of the list column, None where the row is no array; per element a dict {pointer: value} over the
        fields that were found (code 0).  The records come to the host, and the window's bytes, d_idx and d_end once per
        window."""
        col = self.list_column
        off, ok = col.offsets.cpu().tolist(), col.valid.cpu().tolist()
        host = col.window._host_arrays()
        cols = [(pointer, self.column(p)) for p, pointer in enumerate(self.paths.pointers)]
        struct_of = lambda j: {pointer: field_value(c[j], *host) for pointer, c in cols if c[j]["code"] == 0}
        return [[struct_of(j) for j in range(off[k], off[k + 1])] if ok[k] else None for k in range(len(ok))]


class RowSelection(_Records):
    """Rows of a window chosen by predicate, by number or by order ON THE DEVICE (``Window.where``, ``Window.take``,
    ``order_by``): the rows are the chosen documents.  keep bool[D]: the mask over the window's documents (None for
    ``Window.take`` and ``order_by``); rows int32[n_rows]: the chosen documents' numbers -- ascending from ``where``, in the
    order asked for from ``order_by``; fields int64[n_paths, n_rows, 2]: their records, each path a
    column; d_select uint8[48], the ``msj_select_documents_result`` that goes with them.  The methods mean what they mean on
    ``Window``, over the chosen rows: ``raw("", compact=True)`` is the chosen documents as minified NDJSON lines, and
    ``elements`` and ``entries`` give a row per chosen row.  Like every array a Window carries, the window's own arrays are
    reused by the next window."""

    _rows_are = "the chosen rows"

    def __init__(self, window, keep, rows, fields, d_select):
        self.window, self.paths, self.keep, self.rows, self.fields, self.d_select = window, window.paths, keep, rows, fields, d_select

    @property
    def n_rows(self):
        return self.rows.shape[0]

    def number_column(self, path_or_index, dtype=torch.float64):
        """The numbers of one path as ``Window.number_column`` gives them: (values dtype[n_rows], valid bool[n_rows])."""
        return self._number_column(path_or_index, dtype)

    def order_by(self, keys, descending=False, limit=None, cast=None, values_only=False):
        """The chosen rows in the order of one or more paths ON THE DEVICE, as ``Window.order_by`` -> ``RowSelection`` whose
        rows are the window's document numbers in that order; keep is None."""
        order, d_order_select = self.order(keys, limit, cast, values_only, descending)
        fields, d_fsel = self._taken(_or_blank(order, order.shape[0]), d_order_select, order.shape[0])
        return RowSelection(self.window, None, self.rows[order.to(torch.int64)], fields, d_fsel)

    def join(self, other, on, right_on=None, how="inner", by="string", dictionary=None, pairs_capacity=None):
        return _join(self, other, on, right_on, how, by, dictionary, pairs_capacity)


class JoinedRows:
    """The row pairs of an equi-join of two record views ON THE DEVICE (``msj_join_rows_device``; ``Window.join``,
    ``RowSelection.join``).  left / right: a ``RowSelection`` each, over its own window, with one row per PAIR -- pair j is
    row j of both --, so every method of a record view runs on the joined rows: ``joined.right.strings("/name")`` is the
    user's name per event.  right is None for how="semi" / "anti"; for how="left" a left row without a partner has a right
    row of missing values (records with code 20) and the row number -1.  left_rows / right_rows int32[n_pairs]: the pair
    vectors as the call wrote them, row numbers of the two views joined (right_rows -1 where there is none; None for semi /
    anti); offsets int64[L + 1]: the pairs in front of every left row -- with it the pairs are a list column over the left
    rows, a group join; n_pairs; result: the call's ``MsjJoinRowsResult``.  Pairs come in ascending left row and, inside
    one, ascending right row.  BOTH windows must be alive: a window's arrays are reused by its stream's next window."""

    def __init__(self, left, right, left_rows, right_rows, offsets, result):
        self.left, self.right, self.left_rows, self.right_rows, self.offsets, self.result = left, right, left_rows, right_rows, offsets, result

    @property
    def n_pairs(self):
        return self.left_rows.shape[0]

    def to_python(self, paths_left, paths_right=()):
        """The pairs as a list of (left values, right values): a tuple of ``values(path)`` entries per side, the right one
        None for semi / anti.  For tests: both windows come to the host."""
        sides = [list(zip(*[self.left.values(p) for p in paths_left])) if paths_left else [()] * self.n_pairs]
        if self.right is None:
            return [(l, None) for l in sides[0]]
        sides.append(list(zip(*[self.right.values(p) for p in paths_right])) if paths_right else [()] * self.n_pairs)
        return list(zip(*sides))


def _join_keys(view, path, by):
    """The byte column whose equal values are equal join keys"""
    if by == "string":
        return view.strings(path)
    if by == "raw":
        return view.raw(path, compact=True)
    raise ValueError(f'by is "string" or "raw": {by!r}')


def _joined_side(view, d_rows, d_select, n_pairs):
    """One side of the pairs as a ``RowSelection`` over the view's window: its records taken by the pair vector, its rows the
    window's document numbers (-1 where the pair has no row of this side)"""
    fields, d_fsel = view._taken(_or_blank(d_rows, n_pairs), d_select, n_pairs)
    rows = d_rows
    if isinstance(view, RowSelection):
        ok = d_rows >= 0
        at = torch.where(ok, d_rows, torch.zeros_like(d_rows)).to(torch.int64)
        rows = torch.where(ok, _or_blank(view.rows, view.rows.shape[0])[at], torch.full_like(d_rows, -1)) if n_pairs else d_rows
    return RowSelection(view._window, None, rows, fields, d_fsel)


def _join(left, other, on, right_on, how, by, dictionary, pairs_capacity):
    """``Window.join`` / ``RowSelection.join``"""
    if not isinstance(other, (Window, RowSelection)):
        raise TypeError("other is a Window or a RowSelection")
    if how not in _lib.JOIN_KINDS:
        raise ValueError(f"how is one of {sorted(_lib.JOIN_KINDS)}: {how!r}")
    lw, rw = left._window, other._window
    if lw.dev.device != rw.dev.device:
        raise ValueError("the two sides lie on different devices")
    dev = lw.dev
    right_path = on if right_on is None else right_on
    fresh = dictionary is None
    rd = RunningDictionary(dev) if fresh else dictionary
    # the right side first: with a fresh dictionary the left side only looks up, and a value it alone holds is -2, no key
    right_keys = rd.encode(_join_keys(other, right_path, by), what=f"window at {rw.base}: the join keys of {other._rows_are}")
    left_keys = rd.encode(_join_keys(left, on, by), frozen=fresh, what=f"window at {lw.base}: the join keys of {left._rows_are}")
    L, R, G = left_keys.codes.shape[0], right_keys.codes.shape[0], rd.n_distinct
    with_right = how in ("inner", "left")
    room = max(L, 1) if pairs_capacity is None else int(pairs_capacity)
    d_offsets = torch.empty(L + 1, dtype=torch.int64, device=dev.device)
    for _ in range(2):
        res, d_l, d_r, _, d_lsel, d_rsel = dev.join_rows(_or_blank(left_keys.codes, L), _or_blank(right_keys.codes, R), n_keys=G, how=how, left_rows=L,
                                                         right_rows=R, pairs_capacity=room, right=with_right, d_offsets=d_offsets)
        if res.code != errors.CAPACITY or res.n_pairs <= room:
            break
        room = int(res.n_pairs)
    if res.code != 0:
        raise DocumentStreamError(int(res.code), f"window at {lw.base}: {left._rows_are} could not be joined")
    M = int(res.n_pairs)
    d_l = d_l[:M]
    d_r = d_r[:M] if with_right else None
    return JoinedRows(_joined_side(left, d_l, d_lsel, M), _joined_side(other, d_r, d_rsel, M) if with_right else None, d_l, d_r, d_offsets, res)


_JOIN_DOC = """The equi-join of these rows with `other`'s ON THE DEVICE (``msj_dictionary_extend_device`` twice, then
        ``msj_join_rows_device`` and ``msj_take_rows_device``) -> ``JoinedRows``: ``events.join(users, "/user_id", "/id")``
        pairs every event with the user it names.  other: a ``Window`` or ``RowSelection``, of another ``DocumentStream`` on
        the same device or this very window (a self-join).  on / right_on: the key's path on this side and on the other
        (default: the same).  by="string": the key is ``strings(path)``, the unescaped string; a value that is no string is
        no key.  by="raw": the key is ``raw(path, compact=True)``, the value's compact JSON text, so numbers, booleans and
        containers join as well -- by their TEXT: the number 7 matches 7 but neither 7.0 nor "7".  A row without a key
        matches nothing.  how: "inner"; "left" (a row without a partner stays, its right side missing values); "semi" (each
        row with a partner, once); "anti" (each row without one) -- for the last two ``.right`` is None.  Pairs come in the
        order of these rows and, inside one, of the other's.  dictionary: a ``RunningDictionary`` both sides are encoded
        into, so that the windows of a stream joined against one table share the codes; without one a fresh dictionary is
        built from the other side and this side only looked up in it.  pairs_capacity: the first guess of the pairs' room
        (default: these rows); the call is repeated once with what it asks for.  Only the calls' 64-byte results reach the
        host.  BOTH windows must be alive: a window's arrays are reused by its stream's next window."""


def _skip_flag(n):
    return (n & 15) << 24


class DocumentStreamError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"{message} (error {code})")
        self.code = code


@dataclass
class Window(_Records):
    """One window of complete documents, as ``DocumentStream`` yields it.  With select=[...] it is a record view whose rows are
    the window's D = n_documents complete documents: ``column``, ``values``, ``number_column``, ``strings``, ``categories``,
    ``raw``, ``timestamps``, ``parsed_numbers``, ``elements``, ``entries``, ``stats`` and ``order`` by path, and ``cast``,
    ``where``, ``order_by`` and ``take``.  Every array a Window carries is reused by the next window."""
    base: int           # byte offset of the window in the stream (16-byte aligned)
    length: int         # bytes indexed from there
    consumed: int       # bytes that belong to this window's complete documents (the next window starts at base + consumed)
    n_tokens: int       # structurals of the complete documents
    n_documents: int    # complete documents
    utf8_error: bool    # stage 1's UTF-8 verdict for the window (informational unless strict)
    d_idx: torch.Tensor        # int32[n_tokens]: offsets relative to base
    d_type: torch.Tensor       # uint8[n_tokens]
    d_depth: torch.Tensor      # int32[n_tokens]
    d_doc_first: torch.Tensor  # int32[n_documents]: token index of each document's first token
    # DocumentStream(validate=True) only: the rest of stage2_prep's arrays and a verdict per document
    d_match: torch.Tensor = None     # int32[n_tokens]: bracket partners (0xFFFFFFFF: none)
    d_end: torch.Tensor = None       # int32[n_tokens]: end offsets of strings and numbers, relative to base
    d_flags: torch.Tensor = None     # uint8[n_tokens]: MSJ_SPAN_*
    d_verdicts: torch.Tensor = None  # int64[n_documents, 2]: msj_document_verdict -- [k, 0] & 0xFFFFFFFF the code, [k, 1] the error token (-1: none)
    n_invalid: int = None            # documents with a code
    first_invalid: int = None        # the first of them in this window, None if there is none
    verdict_flags: int = None        # MSJ_VALIDATE_* of the window's verdict call
    # DocumentStream(parse=True) only: every document's tape and string buffer (msj_tape_documents_device)
    d_tape: torch.Tensor = None        # int64[tape_words]: document k's tape at [tape_first_k, + tape_words_k)
    d_string_buf: torch.Tensor = None  # uint8[string_bytes]: its string records from string_first_k on
    d_doc_tapes: torch.Tensor = None   # int64[n_documents, 4]: msj_document_tape per document
    n_built: int = None                # documents with code 0: the ones that have a tape
    # DocumentStream(select=[...]) only: a record per (path, document) (msj_select_documents_device)
    d_fields: torch.Tensor = None      # int64[n_paths, n_documents, 2]: msj_field per path and document, each path a column
    d_window: torch.Tensor = None      # uint8[length]: the window's bytes (string fields are spans of them)
    paths: object = None               # the compiled paths (Stage1Device.compile_paths)
    n_found: int = None                # records with code 0, over all paths
    d_select: torch.Tensor = None      # uint8[48]: the select call's msj_select_documents_result, where it lies on the device
    d_docs: torch.Tensor = None        # uint8[32]: the split's msj_documents_result, where it lies on the device
    d_numbers: torch.Tensor = None     # int64[records, 2]: the number call's msj_number records over the window
    d_numbers_result: torch.Tensor = None  # uint8[32]: its msj_numbers_result, where it lies on the device
    dev: object = field(default=None, repr=False, compare=False)  # the Stage1Device whose call strings() runs
    _documents: list = field(default=None, repr=False, compare=False)  # what documents() built: host copies, kept
    _host: tuple = field(default=None, repr=False, compare=False)      # what values() reads: host copies, kept

    _rows_are = "the documents"

    @property
    def _window(self):
        return self

    @property
    def _records(self):
        if self.d_fields is None:
            raise ValueError("no fields: the stream was not created with select=[...]")
        return self.d_fields

    def _token_arrays(self):
        """The token arrays as the calls take them in front of their records"""
        return self.d_idx, self.n_tokens, self.d_type, self.d_depth, self.d_match, self.d_end, self.d_flags

    def _number_records(self):
        """The number call's records and result as the calls take them"""
        return dict(d_numbers=self.d_numbers, numbers_capacity=self.d_numbers.shape[0], d_numbers_result=self.d_numbers_result)

    def _host_arrays(self):
        if self._host is None:
            self._host = (self.d_window.cpu().numpy(), self.d_idx.cpu().numpy().view(np.uint32), self.d_end.cpu().numpy().view(np.uint32))
        return self._host

    def number_column(self, path_or_index, dtype=torch.float64):
        """The numbers of one path as a column ON THE DEVICE, from the records alone (torch operations, no call): (values
        dtype[D], valid bool[D]).  torch.int64: valid where the value is an integer (tag 'l'); torch.float64: the doubles
        (tag 'd') as they are and the integers converted.  A number without bits (MSJ_FIELD_NO_BITS), a value of another
        kind and a record with a code are not valid; their value is 0."""
        return self._number_column(path_or_index, dtype)

    def elements(self, path_or_index, elements_capacity=None):
        """The arrays of one path as a list column ON THE DEVICE -> ``ListColumn``, as every record view's ``elements``; the
        rows being the documents, the call is ``msj_array_column_device``, which finds them by the document split."""
        w, fields, rows, p, what = self._at(path_or_index)
        return _array_elements(w, fields, self.d_select, rows, elements_capacity, None, what, call=lambda d_f, **out: self.dev.array_column(
            *self._token_arrays(), self.d_doc_first, self.d_docs, d_f, p, self.d_select, **self._number_records(), **out))

    def cast(self, path_or_index, kind, unit="ns", keep_numbers=False):
        """One path's strings cast to numbers ON THE DEVICE (``msj_cast_strings_device``) -> (records int64[D, 2], the
        uint8[48] ``msj_select_documents_result`` that goes with them), for callers who chain further: ``filter_rows``,
        ``take_rows`` and ``number_column`` take them as they take a select call's records.  kind: "timestamp" (RFC 3339; the
        int64 counts `unit` since 1970-01-01T00:00:00Z) or "number" (the string, whole, is one JSON number).  A string that is
        neither becomes code 9, a value that is no string code 17 -- or itself, when it is a number and keep_numbers is set."""
        return self._cast_column(path_or_index, kind, unit, keep_numbers)

    def where(self, specs, any=False, cast=None):
        """The documents that pass predicates on their selected fields ON THE DEVICE (``msj_filter_rows_device``,
        ``msj_take_rows_device``) -> ``RowSelection``: ``win.where([("/status", "==", "error"), ("/latency_ms", ">", 250)])``.
        specs: as for ``Stage1Device.compile_predicates`` with the columns named by pointer or index; a string compare is
        on the unescaped value, a number compare exact between int64 and double; ("not", spec) also passes a document
        without the value.  any=True: one predicate is enough.  Only the call's 48-byte result comes to the host.
        cast: ``{"/ts": ("timestamp", "ms"), "/price": "number"}`` makes the predicates see those columns cast
        (``msj_cast_strings_device``), so that ``[("/ts", ">=", t0), ("/ts", "<", t1)]`` is two exact int64 compares; a
        ``datetime.datetime`` operand -- aware, or naive, which means UTC -- becomes the column's unit by integer arithmetic
        (``datetime_units``).  The records the selection carries stay the originals.
        Substring operators on a string column (``msj_match_strings_device`` over its unescaped strings, then "found" on
        the match records): ``("/message", "contains", "timeout")``, ``("/path", "suffix", ".png")``, ``("/line", "like",
        "GET %.png")`` -- % separates literal pieces, a leading or trailing % lifts the anchor, there is no _ --, and
        "icontains" "isuffix" "ilike", which compare A-Z as a-z.  Under ("not", ...) a document without the string passes."""
        keep, kept, d_kept_select, _ = self._filtered(specs, any, cast)
        fields, d_fsel = self._taken(kept, d_kept_select, kept.shape[0])
        return RowSelection(self, keep, kept, fields, d_fsel)

    def order_by(self, keys, descending=False, limit=None, cast=None, values_only=False):
        """The documents in the exact numeric order of one or more paths ON THE DEVICE (``msj_sort_rows_device``,
        ``msj_take_rows_device``) -> ``RowSelection`` with keep None and rows the documents' numbers in that order:
        ``win.order_by("/latency_ms", descending=True, limit=10).raw("", compact=True)`` is the ten slowest lines as
        NDJSON, and ``win.order_by("/ts", cast={"/ts": ("timestamp", "ns")})`` the lines in time order, without the window,
        the column or a count reaching the host.  keys, descending, limit, cast, values_only: as for ``order``."""
        order, d_order_select = self.order(keys, limit, cast, values_only, descending)
        fields, d_fsel = self._taken(_or_blank(order, order.shape[0]), d_order_select, order.shape[0])
        return RowSelection(self, None, order, fields, d_fsel)

    def take(self, rows):
        """The documents with the given numbers ON THE DEVICE (``msj_take_rows_device``) -> ``RowSelection``.  rows: an int32
        device tensor, any order, repeats allowed -- ``categories(path).first`` gives one document per distinct value; a
        number at or past n_documents gives a row of missing values."""
        rows = rows.to(device=self._records.device, dtype=torch.int32).contiguous()
        n = rows.shape[0]
        fields, d_fsel = self._taken(_or_blank(rows, n), _select_word(rows.device, n), n)
        return RowSelection(self, None, rows, fields, d_fsel)

    def join(self, other, on, right_on=None, how="inner", by="string", dictionary=None, pairs_capacity=None):
        return _join(self, other, on, right_on, how, by, dictionary, pairs_capacity)

    def documents(self):
        """A ``Document`` per complete document, None for one with a verdict code (its code: ``d_doc_tapes`` / ``d_verdicts``).
        One copy of the three arrays to the host; the list is kept.  d_tape, d_string_buf and d_doc_tapes are views of
        arrays that the next window reuses, like every array a Window carries: call this before the iterator advances (the
        Documents it returned stay valid, they are host copies)."""
        if self.d_doc_tapes is None:
            raise ValueError("no tapes: the stream was not created with parse=True")
        if self._documents is None:
            recs = np.ascontiguousarray(self.d_doc_tapes.cpu().numpy()).view(DOC_TAPE_DTYPE).reshape(-1)
            tape = self.d_tape.cpu().numpy().view(np.uint64)
            sbuf = self.d_string_buf.cpu().numpy()
            out = []
            for r in recs:
                if r["code"] != 0:
                    out.append(None)
                    continue
                t0, s0 = int(r["tape_first"]), int(r["string_first"])
                out.append(Document(tape[t0:t0 + int(r["tape_words"])], sbuf[s0:s0 + int(r["string_bytes"])]))
            self._documents = out
        return self._documents

    def document(self, k):
        """Document k of the window (None if it has a verdict code)."""
        return self.documents()[k]

    def document_offsets(self):
        """Absolute byte offset of every complete document (host list; reads the device arrays)."""
        first = self.d_doc_first.cpu().numpy().astype("int64")
        idx = self.d_idx.cpu().numpy().view("uint32").astype("int64")
        return [self.base + int(idx[t]) for t in first]


RowSelection.join.__doc__ = Window.join.__doc__ = _JOIN_DOC


class DocumentStream:
    """Iterate over windows of complete documents.

    dev: Stage1Device; d_buf: uint8 device tensor (16-byte aligned) holding the stream; length: bytes;
    window: bytes indexed per step (a document must fit in one window, like upstream's batch_size);
    index_capacity: structurals a window may hold (default: one per byte up to 64 MiB windows, one per
    two bytes beyond).  The arrays a Window carries are reused by the next one.

    validate=True: every window also carries stage 2's verdict for each of its documents
    (``msj_validate_documents_device``, max_depth as there) -- the token pre-pass becomes ``stage2_prep`` with partners, the
    number call and the verdict call follow the split on the same stream, and the small results still come back in one
    read.  Only a window in which the number call found a bad number is visited twice: the number call again with room
    for its records, then the verdict call.  An invalid document is no error of the stream: it is reported in the
    Window.  The window-level errors below stay what they are.

    parse=True (implies validate): every window also carries its documents (``msj_tape_documents_device``):
    ``Window.documents()`` yields a ``Document`` per valid document.  The number call runs with room for its records, the
    tape call follows the verdict call on the same stream, and its 64-byte result comes back in the same read.  The tape,
    the string buffer, the records and the number records start at tape_words / string_bytes / documents / numbers
    (defaults from the index capacity) and grow to what a window needs: the call reports the true sizes, and only the
    calls that need it run again.

    select=[pointers...] (implies validate): every window also carries one ``msj_field`` per pointer and document
    (``msj_select_documents_device``; ``Window.column`` / ``Window.values`` on the host, ``Window.strings`` /
    ``Window.number_column`` / ``Window.elements`` as columns on the device).  The pointers are compiled once, here; the
    number call runs with room for its records, the select call follows the verdict call on the same stream and its
    48-byte result comes back in the same read.  A window with more documents than `documents` records per path grows the
    array and runs only that call again.
    """

    def __init__(self, dev, d_buf, length=None, window=1 << 28, flags=0, index_capacity=None, reuse_counts=True, validate=False,
                 max_depth=100, parse=False, tape_words=None, string_bytes=None, documents=None, numbers=None, select=None):
        self.dev = dev
        self.d_buf = d_buf
        self.length = int(d_buf.numel() if length is None else length)
        self.window = int(min(window, MAX_WINDOW))
        if self.window < 64 or self.window % 16:
            raise ValueError("window must be a multiple of 16 bytes, at least 64")
        if d_buf.data_ptr() % 16:
            raise ValueError("the stream must be 16-byte aligned")
        self.flags = int(flags) & 3
        self.reuse_counts = bool(reuse_counts)  # MSJ_DOCS_AFTER_TOKENS: the split starts from the pre-pass's block counts
        w = min(self.window + 16, max(self.length, 16))
        if index_capacity is None:
            index_capacity = w + 3 if w <= (64 << 20) else w // 2 + 1024
        self.capacity = int(index_capacity)
        dvc = dev.device
        self._idx = torch.empty(self.capacity, dtype=torch.int32, device=dvc)
        self._type = torch.empty(self.capacity, dtype=torch.uint8, device=dvc)
        self._depth = torch.empty(self.capacity, dtype=torch.int32, device=dvc)
        self._first = torch.empty(self.capacity, dtype=torch.int32, device=dvc)
        self._zero = dev.new_carry()
        self._carry = dev.new_carry()
        self.parse = bool(parse)
        self.paths = dev.compile_paths(select) if select is not None else None
        self.validate = bool(validate) or self.parse or self.paths is not None
        self.max_depth = int(max_depth)
        # msj_tokens_result | msj_documents_result (validate: | msj_numbers_result | msj_validate_documents_result; parse:
        # | msj_tape_documents_result; select: | msj_select_documents_result)
        self._sel_at = 208 if self.parse else 144
        size = 208 if self.parse else (144 if self.validate else 64)
        self._results = torch.zeros(size + (48 if self.paths is not None else 0), dtype=torch.uint8, device=dvc)
        if self.validate:
            self._match = torch.empty(self.capacity, dtype=torch.int32, device=dvc)
            self._end = torch.empty(self.capacity, dtype=torch.int32, device=dvc)
            self._flags = torch.empty(self.capacity, dtype=torch.uint8, device=dvc)
            # a verdict per document; documents are a few tokens at the least, and a window with more of them than this
            # (the call says so) grows the array and asks again
            self._verdicts = torch.empty((self.capacity // 8 + 1024, 2), dtype=torch.int64, device=dvc)
        if self.parse:
            cap = self.capacity
            self._tape = torch.empty(max(int(cap + cap // 2 + 2 if tape_words is None else tape_words), 2), dtype=torch.int64, device=dvc)
            self._sbuf = torch.empty(max(int(w + cap // 2 + 64 if string_bytes is None else string_bytes), 16), dtype=torch.uint8, device=dvc)
            self._doc_tapes = torch.empty((max(int(cap // 8 + 1024 if documents is None else documents), 1), 4), dtype=torch.int64, device=dvc)
        if self.parse or self.paths is not None:
            cap = self.capacity
            self._numbers = torch.empty((max(int(cap // 4 + 1024 if numbers is None else numbers), 1), 2), dtype=torch.int64, device=dvc)
        if self.paths is not None:
            rows = max(int(self.capacity // 8 + 1024 if documents is None else documents), 1)
            self._fields = torch.empty((self.paths.n_paths, rows, 2), dtype=torch.int64, device=dvc)
        self.windows = 0

    def __iter__(self):
        dev = self.dev
        pos = 0
        while pos < self.length:
            base = pos & ~15
            skip = pos - base
            wlen = min(self.window + skip, self.length - base)
            last = base + wlen == self.length
            d_win = self.d_buf[base:base + wlen]
            # a window is a non-final shard with zero carries: no return code, no trailer, an unclosed
            # string or a cut UTF-8 character at its end is not an error (the next window starts before it)
            dev.shard(d_win, wlen, self._idx, self._zero, self._carry, is_final=False, flags=self.flags | _skip_flag(skip))
            carry = dev.fetch(self._carry)
            if carry.internal_error:
                raise DocumentStreamError(errors.CAPACITY, f"window at {base}: more than {self.capacity} structurals")
            n = int(carry.count)
            # the two small result structs of the token pre-pass and the split come back in one read
            if self.validate:
                d_type, d_depth, _, d_match, d_end, d_flags = dev.stage2_prep(
                    d_win, wlen, self._idx, n, d_result=self._results[:24], sync=False,
                    arrays=(self._type, self._depth, self._match, self._end, self._flags))
            else:
                d_type, d_depth, _ = dev.tokens(d_win, wlen, self._idx, n, d_type=self._type, d_depth=self._depth,
                                                d_result=self._results[:24], sync=False)
            d_first, _ = dev.documents(d_win, wlen, self._idx, n, d_type, d_depth, is_final=last, d_carry=self._carry,
                                       d_doc_first=self._first, d_result=self._results[32:64], sync=False, after_tokens=self.reuse_counts)
            if self.validate:  # ... and with them those of the number call and the verdict call
                if self.parse or self.paths is not None:  # with room for the records: the tapes and the fields read them
                    d_numbers, ncap = self._numbers, self._numbers.shape[0]
                    dev.number_values(d_win, wlen, self._idx, n, d_flags, capacity=ncap, d_result=self._results[64:96], sync=False,
                                      d_numbers=d_numbers)
                    self._verdict_call(d_win, wlen, n, d_numbers, ncap)
                    if self.parse:
                        self._tape_call(d_win, wlen, n)
                    if self.paths is not None:
                        self._select_call(d_win, wlen, n)
                else:
                    dev.number_values(d_win, wlen, self._idx, n, d_flags, capacity=0, d_result=self._results[64:96], sync=False)
                    self._verdict_call(d_win, wlen, n, None, 0)
            blob = self._results.cpu().numpy().tobytes()
            tok = _lib.MsjTokensResult.from_buffer_copy(blob[:24])
            res = _lib.MsjDocumentsResult.from_buffer_copy(blob[32:64])
            cut = res.n_complete < res.n_documents
            if carry.unescaped_error:
                raise DocumentStreamError(errors.UNESCAPED_CHARS, f"window at {base}: control character inside a string")
            if tok.min_depth < 0:
                raise DocumentStreamError(errors.TAPE_ERROR, f"window at {base}: closing bracket without an opening one")
            if last and cut:
                code = errors.UNCLOSED_STRING if carry.in_string else errors.TAPE_ERROR
                raise DocumentStreamError(code, f"the stream ends inside the document at {base + res.resume_offset}")
            if cut and res.n_complete == 0:
                raise DocumentStreamError(errors.CAPACITY, f"the document at {base + res.resume_offset} does not fit in a window of {self.window} bytes")
            self.windows += 1
            nt, nd = int(res.tokens_complete), int(res.n_complete)
            consumed = int(res.resume_offset) if cut else wlen
            extra = {}
            if self.validate:
                vres = _lib.MsjValidateDocumentsResult.from_buffer_copy(blob[96:144])
                records = self.parse or self.paths is not None
                d_numbers, ncap = (self._numbers, self._numbers.shape[0]) if records else (None, 0)
                numbers_were = self._numbers if records else None
                again = False  # the tape call has to follow a verdict call that ran again
                if vres.code == errors.CAPACITY:  # more documents than verdicts: room for all of them, and once more
                    self._verdicts = torch.empty((nd, 2), dtype=torch.int64, device=dev.device)
                    vres = self._verdict_call(d_win, wlen, n, d_numbers, ncap, read=True)
                    again = True
                if vres.flags & _lib.VALIDATE_NUMBERS_UNCHECKED:
                    # the rare window with a bad number: its records, then the verdicts again
                    cap = _lib.MsjNumbersResult.from_buffer_copy(blob[64:96]).n_numbers
                    if records:
                        self._numbers = torch.empty((cap, 2), dtype=torch.int64, device=dev.device)
                    d_numbers, _ = dev.number_values(d_win, wlen, self._idx, n, d_flags, capacity=cap, d_result=self._results[64:96],
                                                     sync=False, d_numbers=self._numbers if records else None)
                    vres = self._verdict_call(d_win, wlen, n, d_numbers, cap, read=True)
                    again = True
                extra = dict(d_match=d_match[:nt], d_end=d_end[:nt], d_flags=d_flags[:nt], d_verdicts=self._verdicts[:nd],
                             n_invalid=int(vres.n_invalid), verdict_flags=int(vres.flags),
                             first_invalid=int(vres.first_invalid) if vres.n_invalid else None)
                sel_again = again  # ... and so has the select call
                if self.parse:
                    tres = _lib.MsjTapeDocumentsResult.from_buffer_copy(blob[144:208])
                    for _ in range(3):
                        if tres.code == 0 and not again:
                            break
                        tres = self._grow_and_tape(d_win, wlen, n, d_flags, tres)
                        again = False
                    if tres.code != 0:
                        raise DocumentStreamError(int(tres.code), f"window at {base}: the tapes do not fit what the call asked for")
                    extra.update(d_tape=self._tape[:int(tres.tape_words)], d_string_buf=self._sbuf[:int(tres.string_bytes)],
                                 d_doc_tapes=self._doc_tapes[:nd], n_built=int(tres.n_built))
                if self.paths is not None:
                    sres = _lib.MsjSelectDocumentsResult.from_buffer_copy(blob[self._sel_at:self._sel_at + 48])
                    need = _lib.MsjNumbersResult.from_buffer_copy(blob[64:96]).n_numbers
                    if need > self._numbers.shape[0]:  # fewer records than number tokens: the number call again
                        self._numbers = torch.empty((int(need) * 5 // 4 + 1, 2), dtype=torch.int64, device=dev.device)
                        dev.number_values(d_win, wlen, self._idx, n, d_flags, capacity=self._numbers.shape[0], d_result=self._results[64:96],
                                          sync=False, d_numbers=self._numbers)
                    if sres.code == errors.CAPACITY:  # more documents than records per path: room for them, only this call again
                        self._fields = torch.empty((self.paths.n_paths, nd * 5 // 4 + 1, 2), dtype=torch.int64, device=dev.device)
                    if sel_again or sres.code != 0 or self._numbers is not numbers_were:
                        sres = self._select_call(d_win, wlen, n, read=True)
                    if sres.code != 0:
                        raise DocumentStreamError(int(sres.code), f"window at {base}: the fields do not fit what the call asked for")
                    extra.update(d_fields=self._columns[:, :nd], d_window=d_win, paths=self.paths, n_found=int(sres.n_found),
                                 d_select=self._results[self._sel_at:self._sel_at + 48], dev=dev, d_docs=self._results[32:64],
                                 d_numbers=self._numbers, d_numbers_result=self._results[64:96])
            yield Window(base=base, length=wlen, consumed=consumed, n_tokens=nt, n_documents=nd,
                         utf8_error=bool(carry.utf8_error), d_idx=self._idx[:nt], d_type=d_type[:nt],
                         d_depth=d_depth[:nt], d_doc_first=d_first[:nd], **extra)
            pos = base + consumed

    def _verdict_call(self, d_win, wlen, n, d_numbers, numbers_capacity, read=False):
        """``validate_documents`` over the stream's arrays, on the results of the split and the number call where they lie
        on the device; read: wait for its result and return it."""
        r = self._results
        self.dev.validate_documents(d_win, wlen, self._idx, n, self._type, self._depth, self._match, self._end, self._flags,
                                    self._first, r[32:64], d_numbers=d_numbers, numbers_capacity=numbers_capacity,
                                    d_numbers_result=r[64:96], max_depth=self.max_depth, d_verdicts=self._verdicts, d_result=r[96:144],
                                    sync=False)
        if read:
            return _lib.MsjValidateDocumentsResult.from_buffer_copy(r[96:144].cpu().numpy().tobytes())
        return None

    def _tape_call(self, d_win, wlen, n, read=False):
        """``tape_documents`` over the stream's arrays behind the verdict call; read: wait for its result and return it."""
        r = self._results
        # (no more records than verdict rows: the call reads a verdict per document it builds, and builds none when there
        # are more documents than records)
        capacity = min(self._doc_tapes.shape[0], self._verdicts.shape[0])
        self.dev.tape_documents(d_win, wlen, self._idx, n, self._type, self._depth, self._match, self._end, self._flags, self._first,
                                r[32:64], self._numbers, self._numbers.shape[0], d_verdicts=self._verdicts, d_tape=self._tape,
                                d_string_buf=self._sbuf, d_doc_tapes=self._doc_tapes, capacity=capacity, d_result=r[144:208], sync=False)
        if read:
            return _lib.MsjTapeDocumentsResult.from_buffer_copy(r[144:208].cpu().numpy().tobytes())
        return None

    def _select_call(self, d_win, wlen, n, read=False):
        """``select_documents`` over the stream's arrays behind the verdict call; read: wait for its result and return it."""
        r = self._results
        at = self._sel_at
        # (no more records per path than verdict rows: a verdict is read per document looked up.  The records of path p
        # start at p * capacity: the view of the array that the Window carries has that shape)
        capacity = min(self._fields.shape[1], self._verdicts.shape[0])
        n_paths = self.paths.n_paths
        self._columns = self._fields.view(-1, 2)[:n_paths * capacity].view(n_paths, capacity, 2)
        self.dev.select_documents(self.paths, d_win, wlen, self._idx, n, self._type, self._depth, self._match, self._end, self._flags,
                                  self._first, r[32:64], d_numbers=self._numbers, numbers_capacity=self._numbers.shape[0],
                                  d_numbers_result=r[64:96], d_verdicts=self._verdicts, d_fields=self._fields, capacity=capacity,
                                  d_result=r[at:at + 48], sync=False)
        if read:
            return _lib.MsjSelectDocumentsResult.from_buffer_copy(r[at:at + 48].cpu().numpy().tobytes())
        return None

    def _grow_and_tape(self, d_win, wlen, n, d_flags, tres):
        """Room for what the last tape call reported (a quarter more, so that the next window of the kind fits), the number
        call again if its records were too few, then the tape call once more."""
        dvc = self.dev.device
        if tres.tape_words > self._tape.numel():
            self._tape = torch.empty(int(tres.tape_words) * 5 // 4 + 2, dtype=torch.int64, device=dvc)
        if tres.string_bytes > self._sbuf.numel():
            self._sbuf = torch.empty(int(tres.string_bytes) * 5 // 4 + 16, dtype=torch.uint8, device=dvc)
        if tres.n_documents > self._doc_tapes.shape[0]:
            self._doc_tapes = torch.empty((int(tres.n_documents) * 5 // 4 + 1, 4), dtype=torch.int64, device=dvc)
        if tres.n_numbers > self._numbers.shape[0]:
            self._numbers = torch.empty((int(tres.n_numbers) * 5 // 4 + 1, 2), dtype=torch.int64, device=dvc)
            self.dev.number_values(d_win, wlen, self._idx, n, d_flags, capacity=self._numbers.shape[0], d_result=self._results[64:96],
                                   sync=False, d_numbers=self._numbers)
        return self._tape_call(d_win, wlen, n, read=True)
