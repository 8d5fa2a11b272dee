"""Device-resident entry points (what bench.py and the GPU parity tests drive).

PyTorch is plumbing only: it owns device memory (tensors) and the HIP stream;
every byte of the hot path runs in libmsj_stage1.so's HIP kernels through the C
ABI (``msj_stage1_device`` / ``msj_stage1_shard_device``, include/msj_stage1.h).
"""
import ctypes
import struct

import torch

from . import _lib

CARRY_BYTES = 64
SEGMENT_BYTES = 32


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _opt(t):
    """``_ptr`` of a tensor the call can do without: None, a NULL pointer, for None"""
    return None if t is None else _ptr(t)


def _check_records(d_rows, what):
    """``msj_field`` records as int64 of shape (rows, 2) lie back to back"""
    if d_rows.stride(-1) != 1 or (d_rows.shape[0] > 1 and d_rows.stride(0) != 2):
        raise ValueError(f"{what} must be contiguous")


class Paths:
    """Compiled JSON pointers (``msj_paths``), from ``Stage1Device.compile_paths``."""

    def __init__(self, lib, handle, pointers):
        self.lib, self.handle = lib, handle
        self.pointers = [p.decode("utf-8", "surrogateescape") for p in pointers]
        self.n_paths = len(pointers)

    def index(self, path_or_index):
        """The column of a pointer (str) or of an index"""
        if isinstance(path_or_index, (str, bytes)):
            p = path_or_index.decode("utf-8", "surrogateescape") if isinstance(path_or_index, bytes) else path_or_index
            return self.pointers.index(p)
        return range(self.n_paths)[path_or_index]

    def close(self):
        if self.handle:
            self.lib.msj_paths_destroy(self.handle)
            self.handle = None


class Predicates:
    """Compiled row predicates (``msj_predicates``), from ``Stage1Device.compile_predicates``."""

    def __init__(self, lib, handle, n_predicates, max_column, any_):
        self.lib, self.handle = lib, handle
        self.n_predicates, self.max_column, self.any = n_predicates, max_column, any_

    def close(self):
        if self.handle:
            self.lib.msj_predicates_destroy(self.handle)
            self.handle = None


class Patterns:
    """Compiled substring patterns (``msj_patterns``), from ``Stage1Device.compile_patterns``."""

    def __init__(self, lib, handle, n_patterns, max_pieces):
        self.lib, self.handle = lib, handle
        self.n_patterns, self.max_pieces = n_patterns, max_pieces

    def close(self):
        if self.handle:
            self.lib.msj_patterns_destroy(self.handle)
            self.handle = None


def pattern_struct(spec, keep_alive):
    """One spec of ``Stage1Device.compile_patterns`` -> ``_lib.MsjPattern``; the pieces' bytes are appended to keep_alive"""
    if isinstance(spec, (str, bytes, bytearray)):
        spec = ([spec], ())
    if not isinstance(spec, (tuple, list)) or len(spec) != 2 or isinstance(spec[0], (str, bytes, bytearray)) or isinstance(spec[1], (str, bytes)):
        raise ValueError(f"a pattern is bytes / str (contains) or (pieces, flags): {spec!r}")
    pieces = [x.encode("utf-8") if isinstance(x, str) else bytes(x) for x in spec[0]]
    names = list(spec[1])
    if any(n not in _lib.MATCH_FLAGS for n in names):
        raise ValueError(f"a pattern's flags are of {sorted(_lib.MATCH_FLAGS)}: {spec!r}")
    if not 1 <= len(pieces) <= _lib.MATCH_MAX_PIECES or any(not 1 <= len(x) <= _lib.MATCH_MAX_PIECE_BYTES for x in pieces):
        raise ValueError(f"a pattern is 1 to {_lib.MATCH_MAX_PIECES} pieces of 1 to {_lib.MATCH_MAX_PIECE_BYTES} bytes: {spec!r}")
    flags = 0
    for n in names:
        flags |= _lib.MATCH_FLAGS[n]
    data = b"".join(pieces)
    buf = ctypes.create_string_buffer(data, len(data))
    keep_alive.append(buf)
    lens = (ctypes.c_uint32 * 4)(*[len(x) for x in pieces])
    return _lib.MsjPattern(ctypes.addressof(buf), len(pieces), flags, lens)


_TYPE_NAMES = {"object": 1, "array": 2, "string": 4, "int": 8, "double": 16, "number": 8 | 16, "true": 32, "false": 64, "bool": 32 | 64,
               "null": 128}
_NUM_OPS = {"==": _lib.PRED_NUM_EQ, "<": _lib.PRED_NUM_LT, "<=": _lib.PRED_NUM_LE, ">": _lib.PRED_NUM_GT, ">=": _lib.PRED_NUM_GE}
_STR_OPS = {"==": _lib.PRED_STR_EQ, "prefix": _lib.PRED_STR_PREFIX}


def predicate_struct(spec, keep_alive):
    """One spec of ``Stage1Device.compile_predicates`` -> ``_lib.MsjPredicate``; operand bytes are appended to keep_alive"""
    flags = 0
    while len(spec) == 2 and spec[0] == "not":
        flags ^= _lib.PRED_NOT
        spec = spec[1]
    if len(spec) not in (2, 3) or isinstance(spec[0], bool) or not isinstance(spec[0], int) or not isinstance(spec[1], str):
        raise ValueError(f"a predicate is (column, op, operand), (column, 'found') or ('not', predicate): {spec!r}")
    column, op = spec[0], spec[1]
    operand = spec[2] if len(spec) == 3 else None
    if column < 0:
        raise ValueError(f"a column is 0..{_lib.MAX_COLUMNS - 1}: {spec!r}")
    if op == "found" and operand is None:
        return _lib.MsjPredicate(column, _lib.PRED_FOUND, flags, 0, 0, None)
    if op == "type":
        names = [operand] if isinstance(operand, str) else list(operand or ())
        if not names or any(n not in _TYPE_NAMES for n in names):
            raise ValueError(f"a type is one or several of {sorted(_TYPE_NAMES)}: {spec!r}")
        mask = 0
        for n in names:
            mask |= _TYPE_NAMES[n]
        return _lib.MsjPredicate(column, _lib.PRED_TYPE, flags, 0, mask, None)
    if isinstance(operand, bool):
        raise ValueError(f"a bool is no operand (use (column, 'type', 'true')): {spec!r}")
    if isinstance(operand, (str, bytes)) and op in _STR_OPS:
        data = operand.encode("utf-8") if isinstance(operand, str) else bytes(operand)
        buf = ctypes.create_string_buffer(data, max(len(data), 1))
        keep_alive.append(buf)
        return _lib.MsjPredicate(column, _STR_OPS[op], flags, len(data), 0, ctypes.addressof(buf))
    if isinstance(operand, int) and op in _NUM_OPS:
        if not -(1 << 63) <= operand < (1 << 63):
            raise ValueError(f"an int operand is an int64 (write a float for more): {spec!r}")
        return _lib.MsjPredicate(column, _NUM_OPS[op], flags, 0, operand & 0xFFFFFFFFFFFFFFFF, None)
    if isinstance(operand, float) and op in _NUM_OPS:
        bits = int.from_bytes(struct.pack("<d", operand), "little")
        return _lib.MsjPredicate(column, _NUM_OPS[op], flags | _lib.PRED_DOUBLE, 0, bits, None)
    raise ValueError(f"no such predicate: {spec!r}")


class Stage1Device:
    """One ``msj_ctx`` bound to one GPU (one process per GPU)."""

    def __init__(self, device_index=0):
        self.lib = _lib.load()
        if self.lib.msj_device_count() <= 0:
            raise RuntimeError("no HIP device: mojo_simdjson_amd has no CPU fallback")
        self.device_index = device_index
        self.device = torch.device("cuda", device_index)
        h = ctypes.c_void_p()
        rc = self.lib.msj_ctx_create(device_index, ctypes.byref(h))
        if rc != 0:
            raise RuntimeError(f"msj_ctx_create failed: {rc}")
        self.ctx = h
        self._paths = []  # what compile_paths and compile_predicates handed out: closed with the device

    def close(self):
        if self.ctx:
            for paths in self._paths:
                paths.close()
            self._paths = []
            self.lib.msj_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _result(self, d_result=None):
        """The caller's 48-byte result tensor, or a new one"""
        return d_result if d_result is not None else torch.zeros(48, dtype=torch.uint8, device=self.device)

    def _column_rows(self, d_rows, d_offsets, d_valid, capacity):
        """What the column calls default to: capacity = the room of the caller's d_offsets, else the rows of `d_rows`;
        d_offsets: int64[capacity + 1], d_valid: uint8[capacity] (never empty) -> (capacity, d_offsets, d_valid)"""
        if capacity is None:
            capacity = d_offsets.numel() - 1 if d_offsets is not None else d_rows.shape[0]
        capacity = int(capacity)
        if d_offsets is None:
            d_offsets = torch.empty(capacity + 1, dtype=torch.int64, device=self.device)
        if d_valid is None:
            d_valid = torch.empty(max(capacity, 1), dtype=torch.uint8, device=self.device)
        return capacity, d_offsets, d_valid

    def _sized_call(self, call, result_type, d_result, total, wanted, d_outs, room, width, sync):
        """The column calls' way to an output of the right size.  call(room, *d_outs) enqueues the C call with these output
        tensors (None each: layout only) of `room` items; `total` names the field of `result_type` that carries the items the
        call needs; width: 1 for bytes (uint8[room]), 2 for records (int64[room, 2]).  wanted False: the layout-only form
        alone.  Else, without tensors of the caller's (d_outs: a tuple, all given or all None), new ones of `room` items are
        made, and without that number either (None) they are sized from a layout-only first call whose result is waited
        for; with the caller's tensors and no number, what they hold.  -> (the result, or d_result with sync False; d_outs)"""
        def read():
            return result_type.from_buffer_copy(d_result.cpu().numpy().tobytes())

        if not wanted:
            d_outs, room = (None,) * len(d_outs), 0
        elif d_outs[0] is None:
            if room is None:
                call(0, *d_outs)
                room = getattr(read(), total)
            shape, dtype = ((max(int(room), 1),), torch.uint8) if width == 1 else ((max(int(room), 1), 2), torch.int64)
            d_outs = tuple(torch.empty(shape, dtype=dtype, device=self.device) for _ in d_outs)
        elif room is None:
            room = min(t.numel() // width for t in d_outs)
        call(int(room), *d_outs)
        return (read() if sync else d_result), d_outs

    def new_carry(self):
        return torch.zeros(CARRY_BYTES, dtype=torch.uint8, device=self.device)

    def make_carry(self, in_string=0, next_is_escaped=0, prev_scalar=0, count=0, nbytes=0):
        c = _lib.MsjCarry()
        c.in_string, c.next_is_escaped, c.prev_scalar = in_string, next_is_escaped, prev_scalar
        c.count, c.bytes = count, nbytes
        host = torch.frombuffer(bytearray(bytes(c)), dtype=torch.uint8)
        return host.to(self.device)

    def index(self, d_buf, d_idx, d_result, flags=0, length=None):
        """Enqueue stage 1 over a device-resident buffer (asynchronous).

        d_buf: uint8 CUDA tensor (16-byte aligned storage); d_idx: int32/uint32
        CUDA tensor with room for n + 3 entries; d_result: 64-byte CUDA tensor
        receiving the final ``msj_carry`` (count, code, utf8_error ...).
        """
        n = int(d_buf.numel() if length is None else length)
        rc = self.lib.msj_stage1_device(self.ctx, _ptr(d_buf), n, _ptr(d_idx), d_idx.numel(),
                                        _ptr(d_result), self._stream(), flags)
        if rc != 0:  # nothing was enqueued (argument / launch error; 1 = longer than one uint32 segment)
            raise RuntimeError(f"msj_stage1_device failed: {rc}")
        return rc

    def index_types(self, d_buf, d_idx, d_types, d_result, flags=0, length=None):
        """PROTOTYPE (``msj_stage1_types_device``): ``index`` that also writes d_types[k] = d_buf[d_idx[k]] beside every index."""
        n = int(d_buf.numel() if length is None else length)
        rc = self.lib.msj_stage1_types_device(self.ctx, _ptr(d_buf), n, _ptr(d_idx), d_idx.numel(), _ptr(d_types), _ptr(d_result),
                                              self._stream(), flags)
        if rc != 0:
            raise RuntimeError(f"msj_stage1_types_device failed: {rc}")
        return rc

    def stage2_prep_pairs(self, d_buf, length, d_idx, n, spans=True, d_prev=None, d_result=None):
        """``msj_stage2_prep_pairs_device`` (spans=True) / ``msj_tokens_pairs_device``: bracket partners as a compact list --
        d_pairs[k] = (token of the k-th opening bracket, token that closes it or 0xFFFFFFFF) -- instead of an index per
        token.  Returns (d_type, d_depth, d_pairs int32[n_cap, 2], d_end or None, d_flags or None, d_result); asynchronous:
        the number of records is msj_tokens_result.reserved."""
        n = int(n)
        dv = self.device
        d_type = torch.empty(max(n, 8), dtype=torch.uint8, device=dv)
        d_depth = torch.empty(max(n, 4), dtype=torch.int32, device=dv)
        d_pairs = torch.empty((max(n, 1), 2), dtype=torch.int32, device=dv)
        d_res = d_result if d_result is not None else torch.zeros(24, dtype=torch.uint8, device=dv)
        prev = _opt(d_prev)
        if spans:
            d_end = torch.empty(max(n, 2), dtype=torch.int32, device=dv)
            d_flags = torch.empty(max(n, 2), dtype=torch.uint8, device=dv)
            rc = self.lib.msj_stage2_prep_pairs_device(self.ctx, _ptr(d_buf), int(length), _ptr(d_idx), n, _ptr(d_type), _ptr(d_depth),
                                                       _ptr(d_pairs), _ptr(d_end), _ptr(d_flags), _ptr(d_res), prev, self._stream())
        else:
            d_end = d_flags = None
            rc = self.lib.msj_tokens_pairs_device(self.ctx, _ptr(d_buf), int(length), _ptr(d_idx), n, _ptr(d_type), _ptr(d_depth),
                                                  _ptr(d_pairs), _ptr(d_res), prev, self._stream())
        if rc != 0:
            raise RuntimeError(f"msj_*_pairs_device failed: {rc}")
        return d_type[:n], d_depth[:n], d_pairs, d_end, d_flags, d_res

    def depth_from_types(self, d_type, n, d_depth=None, d_match=None, match=False, d_result=None, d_prev=None):
        """PROTOTYPE (``msj_depth_from_types_device``): depth (and partners) of every token from type bytes stage 1 wrote.
        Asynchronous; returns (d_depth, d_match or None, d_result)."""
        n = int(n)
        if d_depth is None:
            d_depth = torch.empty(max(n, 4), dtype=torch.int32, device=self.device)
        if match and d_match is None:
            d_match = torch.empty(max(n, 4), dtype=torch.int32, device=self.device)
        d_res = d_result if d_result is not None else torch.zeros(24, dtype=torch.uint8, device=self.device)
        rc = self.lib.msj_depth_from_types_device(self.ctx, _ptr(d_type), n, _ptr(d_depth), _opt(d_match),
                                                  _ptr(d_res), _opt(d_prev), self._stream())
        if rc != 0:
            raise RuntimeError(f"msj_depth_from_types_device failed: {rc}")
        return d_depth, d_match, d_res

    def shard(self, d_buf, length, d_idx, carry_in, carry_out, segments=None, has_prefix=False,
              is_final=False, no_emit=False, trailer_len=0, flags=0):
        nseg = ctypes.c_uint32(0)
        rc = self.lib.msj_stage1_shard_device(
            self.ctx, _ptr(d_buf), int(length),
            _opt(d_idx),
            d_idx.numel() if d_idx is not None else 0,
            _ptr(carry_in), _ptr(carry_out),
            _opt(segments),
            (segments.numel() // SEGMENT_BYTES) if segments is not None else 0,
            ctypes.byref(nseg), int(has_prefix), int(is_final), int(no_emit), int(trailer_len),
            self._stream(), flags)
        if rc != 0:  # nothing (or not everything) was enqueued
            raise RuntimeError(f"msj_stage1_shard_device failed: {rc}")
        return rc, nseg.value

    def tokens(self, d_buf, length, d_idx, n, d_type=None, d_depth=None, d_match=None, match=False, d_result=None, sync=True,
               d_prev=None):
        """Token stream for stage 2 (``msj_tokens_device``): type byte and nesting depth of every
        structural, optionally (match=True or d_match given) the partner index of every bracket.
        Returns (d_type uint8[n], d_depth int32[n], msj_tokens_result[, d_match int32[n]]); blocking
        only for the 24-byte result (sync=False: not at all, the result stays in d_result on the device)."""
        n = int(n)
        if d_type is None:
            d_type = torch.empty(max(n, 1), dtype=torch.uint8, device=self.device)
        if d_depth is None:
            d_depth = torch.empty(max(n, 1), dtype=torch.int32, device=self.device)
        if match and d_match is None:
            d_match = torch.empty(max(n, 1), dtype=torch.int32, device=self.device)
        d_res = d_result if d_result is not None else torch.zeros(24, dtype=torch.uint8, device=self.device)
        # d_prev: the device msj_tokens_result of the call for the tokens in front (``msj_tokens_chain_device``)
        rc = self.lib.msj_tokens_chain_device(self.ctx, _ptr(d_buf), int(length), _ptr(d_idx), n, _ptr(d_type),
                                              _ptr(d_depth), _opt(d_match),
                                              _ptr(d_res), _opt(d_prev), self._stream())
        if rc != 0:
            raise RuntimeError(f"msj_tokens_device failed: {rc}")
        # sync=False: nothing is waited for; the third element is the device tensor holding the msj_tokens_result
        res = _lib.MsjTokensResult.from_buffer_copy(d_res.cpu().numpy().tobytes()) if sync else d_res
        if d_match is not None:
            return d_type[:n], d_depth[:n], res, d_match[:n]
        return d_type[:n], d_depth[:n], res

    def token_spans(self, d_buf, length, d_idx, n):
        """Closing quote / escape flag of every string token, end / float flag of every number token
        (``msj_token_spans_device``).  Returns (d_end int32[n] viewed as uint32, d_flags uint8[n]); asynchronous."""
        n = int(n)
        d_end = torch.empty(max(n, 1), dtype=torch.int32, device=self.device)
        d_flags = torch.empty(max(n, 1), dtype=torch.uint8, device=self.device)
        rc = self.lib.msj_token_spans_device(self.ctx, _ptr(d_buf), int(length), _ptr(d_idx), n, _ptr(d_end),
                                             _ptr(d_flags), self._stream())
        if rc != 0:
            raise RuntimeError(f"msj_token_spans_device failed: {rc}")
        return d_end[:n], d_flags[:n]

    def stage2_prep(self, d_buf, length, d_idx, n, match=False, d_prev=None, d_result=None, arrays=None, sync=True):
        """``tokens`` and ``token_spans`` in one go (``msj_stage2_prep_device``), identical results:
        returns (d_type, d_depth, msj_tokens_result, d_match or None, d_end, d_flags).  d_prev: the device
        msj_tokens_result of the call for the tokens in front (``msj_stage2_prep_chain_device``); d_result: where
        this call's goes (to hand on as the next call's d_prev).  arrays: (d_type, d_depth, d_match or None, d_end,
        d_flags) of the caller's to write into, at least n long; sync=False: nothing is waited for, the third element is
        the device tensor that holds the result."""
        n = int(n)
        dv = self.device
        if arrays is not None:
            d_type, d_depth, d_match, d_end, d_flags = arrays
            match = d_match is not None
        else:
            d_type = torch.empty(max(n, 1), dtype=torch.uint8, device=dv)
            d_depth = torch.empty(max(n, 1), dtype=torch.int32, device=dv)
            d_match = torch.empty(max(n, 1), dtype=torch.int32, device=dv) if match else None
            d_end = torch.empty(max(n, 1), dtype=torch.int32, device=dv)
            d_flags = torch.empty(max(n, 1), dtype=torch.uint8, device=dv)
        d_res = d_result if d_result is not None else torch.zeros(24, dtype=torch.uint8, device=dv)
        rc = self.lib.msj_stage2_prep_chain_device(self.ctx, _ptr(d_buf), int(length), _ptr(d_idx), n, _ptr(d_type), _ptr(d_depth),
                                                   _ptr(d_match) if match else None, _ptr(d_end), _ptr(d_flags), _ptr(d_res),
                                                   _opt(d_prev), self._stream())
        if rc != 0:
            raise RuntimeError(f"msj_stage2_prep_device failed: {rc}")
        res = _lib.MsjTokensResult.from_buffer_copy(d_res.cpu().numpy().tobytes()) if sync else d_res
        return d_type[:n], d_depth[:n], res, (d_match[:n] if match else None), d_end[:n], d_flags[:n]

    def stage2_prep_segments(self, d_buf, segments, d_idx, match=False, d_prev=None):
        """Rows f1 + f2 + f4 for a shard of several uint32 segments (``msj_stage2_prep_segments``).  segments: list of
        (byte_base, byte_len, index_begin, count) -- a host copy of the msj_segment table the shard call wrote.
        Returns (offsets, d_type, d_depth, d_match or None, d_end, d_flags, results): segment s's arrays are the slices
        [offsets[s], offsets[s] + count_s); results = one msj_tokens_result per segment (the last describes the shard)."""
        nseg = len(segments)
        table = (_lib.MsjSegment * nseg)()
        for k, (bb, bl, ib, cnt) in enumerate(segments):
            table[k].byte_base, table[k].byte_len, table[k].index_begin, table[k].count = bb, bl, ib, cnt
        total = sum(((c + 7) // 8) * 8 for _, _, _, c in segments)
        dv = self.device
        d_type = torch.empty(max(total, 8), dtype=torch.uint8, device=dv)
        d_depth = torch.empty(max(total, 8), dtype=torch.int32, device=dv)
        d_match = torch.empty(max(total, 8), dtype=torch.int32, device=dv) if match else None
        d_end = torch.empty(max(total, 8), dtype=torch.int32, device=dv)
        d_flags = torch.empty(max(total, 8), dtype=torch.uint8, device=dv)
        d_res = torch.zeros(24 * nseg, dtype=torch.uint8, device=dv)
        offs = (ctypes.c_uint64 * nseg)()
        rc = self.lib.msj_stage2_prep_segments(self.ctx, _ptr(d_buf), ctypes.byref(table), nseg, _ptr(d_idx), _ptr(d_type), _ptr(d_depth),
                                               _ptr(d_match) if match else None, _ptr(d_end), _ptr(d_flags), _ptr(d_res),
                                               _opt(d_prev), offs, self._stream())
        if rc != 0:
            raise RuntimeError(f"msj_stage2_prep_segments failed: {rc}")
        raw = d_res.cpu().numpy().tobytes()
        results = [_lib.MsjTokensResult.from_buffer_copy(raw[24 * k: 24 * k + 24]) for k in range(nseg)]
        return [int(o) for o in offs], d_type, d_depth, d_match, d_end, d_flags, results

    def documents(self, d_buf, length, d_idx, n, d_type, d_depth, is_final=False, d_carry=None, d_doc_first=None,
                  d_result=None, sync=True, after_tokens=False):
        """Document split of one window of a stream of concatenated documents (``msj_documents_device``):
        the token index at which each document starts, and how far the complete documents reach.
        d_buf / length: the window; is_final: it ends the stream; d_type / d_depth: from ``tokens`` for the
        same d_idx; d_carry: the window's stage-1 carry_out; after_tokens: d_type / d_depth are what the last
        ``tokens`` / ``stage2_prep`` call of this device wrote, untouched since (MSJ_DOCS_AFTER_TOKENS).
        Returns (d_doc_first int32[capacity], msj_documents_result) -- blocking for the 32-byte result --
        or, with sync=False, (d_doc_first, d_result) with nothing waited for."""
        n = int(n)
        if d_doc_first is None:
            d_doc_first = torch.empty(max(n, 1), dtype=torch.int32, device=self.device)
        if d_result is None:
            d_result = torch.zeros(32, dtype=torch.uint8, device=self.device)
        rc = self.lib.msj_documents_device(self.ctx, _ptr(d_buf), int(length), int(bool(is_final)) | (2 if after_tokens else 0), _ptr(d_idx), n,
                                           _ptr(d_type),
                                           _ptr(d_depth), _opt(d_carry), _ptr(d_doc_first),
                                           d_doc_first.numel(), _ptr(d_result), self._stream())
        if rc != 0:
            raise RuntimeError(f"msj_documents_device failed: {rc}")
        if not sync:
            return d_doc_first, d_result
        return d_doc_first, _lib.MsjDocumentsResult.from_buffer_copy(d_result.cpu().numpy().tobytes())

    def number_values(self, d_buf, length, d_idx, n, d_flags, capacity=None, d_result=None, sync=True, d_numbers=None):
        """Values of the number tokens (``msj_number_values_device``): one 16-byte ``msj_number`` record per token whose
        d_flags (from ``token_spans`` / ``stage2_prep*`` for the same d_idx) has MSJ_SPAN_NUMBER, in token order -- the exact
        int64 or the nearest binary64, or a syntax / range error.  capacity: records stored at most (default n).
        Returns (d_numbers, msj_numbers_result) -- d_numbers an int64 tensor of shape (capacity, 2): [k, 0] the bits,
        [k, 1] token | kind << 32 -- blocking for the 32-byte result; with sync=False (d_numbers, d_result) with nothing
        waited for.  d_numbers: a tensor of that shape to write into instead of a new one (at least `capacity` rows)."""
        n = int(n)
        capacity = n if capacity is None else int(capacity)
        if d_numbers is None:
            d_numbers = torch.empty((max(capacity, 1), 2), dtype=torch.int64, device=self.device)
        if d_result is None:
            d_result = torch.zeros(32, dtype=torch.uint8, device=self.device)
        rc = self.lib.msj_number_values_device(self.ctx, _ptr(d_buf), int(length), _ptr(d_idx), n, _ptr(d_flags), _ptr(d_numbers),
                                               capacity, _ptr(d_result), self._stream())
        if rc != 0:
            raise RuntimeError(f"msj_number_values_device failed: {rc}")
        if not sync:
            return d_numbers, d_result
        return d_numbers, _lib.MsjNumbersResult.from_buffer_copy(d_result.cpu().numpy().tobytes())

    def validate(self, d_buf, length, d_idx, n, d_type, d_depth, d_match, d_end, d_flags, d_numbers_result=None, max_depth=100,
                 d_result=None, sync=True):
        """Stage 2's verdict for one document (``msj_validate_device``): the code and the token at which the reference's
        ``walk_document`` would stop.  The arrays are what ``stage2_prep(match=True)`` wrote for the same d_idx;
        d_numbers_result: the device ``msj_numbers_result`` of ``number_values(..., sync=False)`` over the same tokens (None:
        numbers are not checked, MSJ_VALIDATE_NUMBERS_UNCHECKED is set).  Returns the ``MsjValidateResult`` -- blocking for
        its 32 bytes; with sync=False the device tensor that holds it, nothing waited for."""
        if d_result is None:
            d_result = torch.zeros(32, dtype=torch.uint8, device=self.device)
        rc = self.lib.msj_validate_device(self.ctx, _ptr(d_buf), int(length), _ptr(d_idx), int(n), _ptr(d_type), _ptr(d_depth),
                                          _ptr(d_match), _ptr(d_end), _ptr(d_flags),
                                          _opt(d_numbers_result), int(max_depth),
                                          _ptr(d_result), self._stream())
        if rc != 0:
            raise RuntimeError(f"msj_validate_device failed: {rc}")
        if not sync:
            return d_result
        return _lib.MsjValidateResult.from_buffer_copy(d_result.cpu().numpy().tobytes())

    def validate_documents(self, d_buf, length, d_idx, n, d_type, d_depth, d_match, d_end, d_flags, d_doc_first, d_docs,
                           d_numbers=None, numbers_capacity=0, d_numbers_result=None, max_depth=100, d_verdicts=None, capacity=None,
                           d_result=None, sync=True):
        """A verdict for every complete document of a window (``msj_validate_documents_device``): what ``validate`` gives
        for each document's token sub-arrays, in one pass over the window.  The arrays are what ``stage2_prep(match=True)``
        wrote for the window's d_idx; d_doc_first / d_docs: the device arrays of ``documents(..., sync=False)`` over them (how
        many documents there are is read on the device); d_numbers / d_numbers_result: from ``number_values(..., sync=False)``
        -- no record is needed unless that call found an error (capacity 0 will do; MSJ_VALIDATE_NUMBERS_UNCHECKED in the
        result's flags says that the records are wanted).  d_verdicts: int64 tensor of shape (capacity, 2) -- [k, 0] the code
        in its low 32 bits, [k, 1] the error token, -1 for none -- default one row per token.  Returns (d_verdicts,
        ``MsjValidateDocumentsResult``) -- blocking for the 48-byte result; with sync=False (d_verdicts, d_result) with
        nothing waited for."""
        n = int(n)
        if d_verdicts is None:
            capacity = n if capacity is None else int(capacity)
            d_verdicts = torch.empty((max(capacity, 1), 2), dtype=torch.int64, device=self.device)
        elif capacity is None:
            capacity = d_verdicts.shape[0]
        if d_result is None:
            d_result = torch.zeros(48, dtype=torch.uint8, device=self.device)
        rc = self.lib.msj_validate_documents_device(
            self.ctx, _ptr(d_buf), int(length), _ptr(d_idx), n, _ptr(d_type), _ptr(d_depth), _ptr(d_match), _ptr(d_end), _ptr(d_flags),
            _ptr(d_doc_first), _ptr(d_docs), _opt(d_numbers if numbers_capacity else None), int(numbers_capacity),
            _opt(d_numbers_result), int(max_depth), _ptr(d_verdicts), int(capacity),
            _ptr(d_result), self._stream())
        if rc != 0:
            raise RuntimeError(f"msj_validate_documents_device failed: {rc}")
        if not sync:
            return d_verdicts, d_result
        return d_verdicts, _lib.MsjValidateDocumentsResult.from_buffer_copy(d_result.cpu().numpy().tobytes())

    def validate_document(self, d_buf, length, max_depth=100):
        """Is this device buffer one valid JSON document, and if not, which error and where: stage 1, ``stage2_prep`` with
        partners, ``number_values`` and ``validate`` enqueued on one stream.  Returns stage 1's code if that is not 0, else
        the ``MsjValidateResult``.  (The token count sizes the later launches: it is the one value read in between.)"""
        length = int(length)
        d_idx = torch.empty(length + 3 + 4, dtype=torch.int32, device=self.device)
        d_carry = self.new_carry()
        self.index(d_buf, d_idx, d_carry, length=length)
        carry = self.fetch(d_carry)
        if carry.code != 0:
            return int(carry.code)
        n = int(carry.count)
        d_type, d_depth, _, d_match, d_end, d_flags = self.stage2_prep(d_buf, length, d_idx, n, match=True)
        _, d_num = self.number_values(d_buf, length, d_idx, n, d_flags, capacity=0, sync=False)
        return self.validate(d_buf, length, d_idx, n, d_type, d_depth, d_match, d_end, d_flags, d_num, max_depth)

    def tape(self, d_buf, length, d_idx, n, d_type, d_depth, d_match, d_end, d_flags, d_numbers, numbers_capacity, d_verdict=None,
             d_tape=None, tape_capacity=None, d_string_buf=None, string_capacity=None, strings=True, d_result=None, sync=True):
        """The document's tape and string buffer (``msj_tape_device``).  The arrays are what ``stage2_prep(match=True)`` and
        ``number_values`` wrote for the same d_idx; d_verdict: the device ``msj_validate_result`` (``validate(..., sync=False)``),
        read on the device -- a code other than 0 ends the call with that code.  d_tape: int64 tensor (default: one of
        ``tape_capacity`` words, default n + numbers_capacity + 2, always enough); d_string_buf: uint8 tensor (default: one of
        ``string_capacity`` bytes, default the reference's bound 5 * length // 3 + 64); strings=False: the layout-only form
        (d_string_buf NULL).  Returns (``MsjTapeResult``, d_tape, d_string_buf) -- blocking for the 32-byte result; with
        sync=False the device tensor that holds it, nothing waited for."""
        n, length, numbers_capacity = int(n), int(length), int(numbers_capacity)
        if d_tape is None:
            tape_capacity = n + numbers_capacity + 2 if tape_capacity is None else int(tape_capacity)
            d_tape = torch.empty(max(tape_capacity, 2), dtype=torch.int64, device=self.device)
        elif tape_capacity is None:
            tape_capacity = d_tape.numel()
        if not strings:
            d_string_buf, string_capacity = None, 0
        elif d_string_buf is None:
            string_capacity = 5 * length // 3 + 64 if string_capacity is None else int(string_capacity)
            d_string_buf = torch.empty(max(string_capacity, 1), dtype=torch.uint8, device=self.device)
        elif string_capacity is None:
            string_capacity = d_string_buf.numel()
        if d_result is None:
            d_result = torch.zeros(32, dtype=torch.uint8, device=self.device)
        rc = self.lib.msj_tape_device(self.ctx, _ptr(d_buf), length, _ptr(d_idx), n, _ptr(d_type), _ptr(d_depth), _ptr(d_match),
                                      _ptr(d_end), _ptr(d_flags), _opt(d_numbers),
                                      numbers_capacity, None, _opt(d_verdict), _ptr(d_tape),
                                      int(tape_capacity), _opt(d_string_buf),
                                      int(string_capacity), _ptr(d_result), self._stream())
        if rc != 0:
            raise RuntimeError(f"msj_tape_device failed: {rc}")
        if not sync:
            return d_result, d_tape, d_string_buf
        return _lib.MsjTapeResult.from_buffer_copy(d_result.cpu().numpy().tobytes()), d_tape, d_string_buf

    def tape_documents(self, d_buf, length, d_idx, n, d_type, d_depth, d_match, d_end, d_flags, d_doc_first, d_docs, d_numbers,
                       numbers_capacity, d_verdicts=None, d_tape=None, tape_capacity=None, d_string_buf=None, string_capacity=None,
                       strings=True, d_doc_tapes=None, capacity=None, d_result=None, sync=True):
        """A tape and a string buffer for every complete document of a window (``msj_tape_documents_device``): what ``tape``
        gives for each document's token sub-arrays, in one pass over the window.  The arrays are what
        ``stage2_prep(match=True)`` wrote for the window's d_idx; d_doc_first / d_docs: the device arrays of
        ``documents(..., sync=False)``; d_numbers: the records of ``number_values`` over the whole window; d_verdicts: the
        rows of ``validate_documents`` (None: every document is built).  d_tape: int64 tensor (default: one of
        ``tape_capacity`` words, default 3 * n + 2, always enough); d_string_buf: uint8 tensor (default: one of
        ``string_capacity`` bytes, default 5 * length // 3 + 4 * n + 64); strings=False: the layout-only form; d_doc_tapes:
        int64 tensor of shape (capacity, 4), one ``msj_document_tape`` per row (default one row per token).  Returns
        (``MsjTapeDocumentsResult``, d_tape, d_string_buf, d_doc_tapes) -- blocking for the 64-byte result; with sync=False
        the device tensor that holds it, nothing waited for."""
        n, length, numbers_capacity = int(n), int(length), int(numbers_capacity)
        if d_tape is None:
            tape_capacity = 3 * n + 2 if tape_capacity is None else int(tape_capacity)
            d_tape = torch.empty(max(tape_capacity, 2), dtype=torch.int64, device=self.device)
        elif tape_capacity is None:
            tape_capacity = d_tape.numel()
        if not strings:
            d_string_buf, string_capacity = None, 0
        elif d_string_buf is None:
            string_capacity = 5 * length // 3 + 4 * n + 64 if string_capacity is None else int(string_capacity)
            d_string_buf = torch.empty(max(string_capacity, 1), dtype=torch.uint8, device=self.device)
        elif string_capacity is None:
            string_capacity = d_string_buf.numel()
        if d_doc_tapes is None:
            capacity = n if capacity is None else int(capacity)
            d_doc_tapes = torch.empty((max(capacity, 1), 4), dtype=torch.int64, device=self.device)
        elif capacity is None:
            capacity = d_doc_tapes.shape[0]
        if d_result is None:
            d_result = torch.zeros(64, dtype=torch.uint8, device=self.device)
        rc = self.lib.msj_tape_documents_device(
            self.ctx, _ptr(d_buf), length, _ptr(d_idx), n, _ptr(d_type), _ptr(d_depth), _ptr(d_match), _ptr(d_end), _ptr(d_flags),
            _ptr(d_doc_first), _ptr(d_docs), _opt(d_numbers if numbers_capacity else None), numbers_capacity,
            None, _opt(d_verdicts), _ptr(d_tape), int(tape_capacity),
            _opt(d_string_buf), int(string_capacity), _ptr(d_doc_tapes), int(capacity),
            _ptr(d_result), self._stream())
        if rc != 0:
            raise RuntimeError(f"msj_tape_documents_device failed: {rc}")
        if not sync:
            return d_result, d_tape, d_string_buf, d_doc_tapes
        return _lib.MsjTapeDocumentsResult.from_buffer_copy(d_result.cpu().numpy().tobytes()), d_tape, d_string_buf, d_doc_tapes

    def compile_paths(self, pointers):
        """Compile RFC 6901 JSON pointers -- object keys only, "" the root value; 1 to 16 of them, at most 8 segments of at
        most 255 bytes each -- for ``select_documents`` (``msj_paths_create``).  pointers: str (UTF-8) or bytes.  The handle
        is immutable, usable by any number of calls, and closed with the device.  ValueError for a pointer that is none
        (INVALID_JSON_POINTER) or beyond the limits."""
        pointers = [p.encode("utf-8") if isinstance(p, str) else bytes(p) for p in pointers]
        if any(b"\0" in p for p in pointers):
            raise ValueError("a JSON pointer cannot hold a NUL byte")
        table = (ctypes.c_char_p * max(len(pointers), 1))(*pointers)
        h = ctypes.c_void_p()
        rc = self.lib.msj_paths_create(self.ctx, table, len(pointers), ctypes.byref(h))
        if rc == _lib.INVALID_JSON_POINTER:
            raise ValueError(f"not a JSON pointer (error {rc}): {pointers}")
        if rc == -1:
            raise ValueError(f"1 to {_lib.MAX_PATHS} paths of at most {_lib.MAX_PATH_SEGMENTS} segments of at most "
                             f"{_lib.MAX_SEGMENT_BYTES} bytes: {pointers}")
        if rc != 0:
            raise RuntimeError(f"msj_paths_create failed: {rc}")
        paths = Paths(self.lib, h, pointers)
        self._paths.append(paths)
        return paths

    def select_documents(self, paths, d_buf, length, d_idx, n, d_type, d_depth, d_match, d_end, d_flags, d_doc_first, d_docs,
                         d_numbers=None, numbers_capacity=0, d_numbers_result=None, d_verdicts=None, d_fields=None, capacity=None,
                         d_result=None, sync=True):
        """Fields by path for every complete document of a window (``msj_select_documents_device``): one 16-byte
        ``msj_field`` per (path, document), path-major.  paths: from ``compile_paths``; the arrays as for ``tape_documents``;
        d_numbers / d_numbers_result: the records and the device result of ``number_values`` over the whole window (without
        them a number field has its tag and MSJ_FIELD_NO_BITS); d_verdicts: the rows of ``validate_documents`` (None: every
        document is looked up).  d_fields: int64 tensor of shape (n_paths, capacity, 2) -- [p, k, 0] the bits, [p, k, 1]
        token | type << 32 | flags << 40 | code << 48 -- default one row per token.  Returns (``MsjSelectDocumentsResult``,
        d_fields) -- blocking for the 48-byte result; with sync=False the device tensor that holds it, nothing waited for."""
        n, length, numbers_capacity = int(n), int(length), int(numbers_capacity)
        if d_fields is None:
            capacity = n if capacity is None else int(capacity)
            d_fields = torch.empty((paths.n_paths, max(capacity, 1), 2), dtype=torch.int64, device=self.device)
        elif capacity is None:
            capacity = d_fields.shape[1]
        if d_result is None:
            d_result = torch.zeros(48, dtype=torch.uint8, device=self.device)
        rc = self.lib.msj_select_documents_device(
            self.ctx, paths.handle, _ptr(d_buf), length, _ptr(d_idx), n, _ptr(d_type), _ptr(d_depth), _ptr(d_match), _ptr(d_end), _ptr(d_flags),
            _ptr(d_doc_first), _ptr(d_docs), _opt(d_numbers if numbers_capacity else None), numbers_capacity,
            _opt(d_numbers_result), _opt(d_verdicts),
            _ptr(d_fields), int(capacity), _ptr(d_result), self._stream())
        if rc != 0:
            raise RuntimeError(f"msj_select_documents_device failed: {rc}")
        if not sync:
            return d_result, d_fields
        return _lib.MsjSelectDocumentsResult.from_buffer_copy(d_result.cpu().numpy().tobytes()), d_fields

    def string_column(self, d_buf, length, d_fields, p, d_select_result, d_offsets=None, d_valid=None, d_bytes=None, capacity=None,
                      bytes_capacity=None, strings=True, d_result=None, sync=True):
        """One path's string values as a column (``msj_string_column_device``): offsets, the unescaped bytes back to back
        and a validity byte per row, all on the device.  d_buf / length: the window ``select_documents`` ran over; d_fields:
        its records, int64 of shape (n_paths, rows, 2); p: the path's index; d_select_result: the device
        ``msj_select_documents_result`` of that call (``select_documents(..., sync=False)``), read on the device.  d_offsets:
        int64 tensor of capacity + 1 entries, d_valid: uint8 tensor of capacity entries (default: new ones, capacity = the
        rows of d_fields); d_bytes: uint8 tensor of ``bytes_capacity`` bytes (default: its size).  Without a d_bytes of the
        caller's, one of ``bytes_capacity`` bytes is made, and without that number either it is sized from a layout-only
        first call, whose 48-byte result is waited for.  strings=False: the layout-only form alone (d_bytes None).  Returns
        (``MsjStringColumnResult``, d_offsets, d_valid, d_bytes) -- blocking for the 48-byte result; with sync=False the
        device tensor that holds it, nothing waited for."""
        d_col = d_fields[p]
        _check_records(d_col, "the records of a path")
        capacity, d_offsets, d_valid = self._column_rows(d_col, d_offsets, d_valid, capacity)
        d_result = self._result(d_result)

        def call(room, d_out):
            rc = self.lib.msj_string_column_device(self.ctx, _ptr(d_buf), int(length), _ptr(d_col), _ptr(d_select_result), _ptr(d_offsets),
                                                   _ptr(d_valid), capacity, _opt(d_out), room, _ptr(d_result), self._stream())
            if rc != 0:
                raise RuntimeError(f"msj_string_column_device failed: {rc}")

        res, (d_bytes,) = self._sized_call(call, _lib.MsjStringColumnResult, d_result, "total_bytes", strings, (d_bytes,), bytes_capacity, 1, sync)
        return res, d_offsets, d_valid, d_bytes

    def raw_column(self, d_buf, length, d_idx, n, d_type, d_match, d_end, d_flags, d_rows, d_rows_select, d_offsets=None, d_valid=None,
                   d_bytes=None, capacity=None, bytes_capacity=None, compact=False, text=True, d_result=None, sync=True):
        """The JSON text of the values that records name, as a column (``msj_raw_column_device``): offsets, the text back to
        back and a validity byte per row, all on the device.  d_buf / length and the token arrays: the window the records
        were written over; d_rows: int64 of shape (rows, 2), any ``msj_field`` records in any order -- a path of
        ``select_documents`` or ``select_elements``, the elements of a list column, the keys or values of a map column;
        d_rows_select: the device ``msj_select_documents_result`` that counts them, read on the device.  compact=False: the
        window's bytes from the value's first to its last; compact=True (MSJ_RAW_COMPACT): the blanks between tokens
        dropped.  d_offsets, d_valid, d_bytes, capacity, bytes_capacity and the layout-only first call when no size is given
        are ``string_column``'s; text=False: the layout-only form alone (d_bytes None).  Returns (``MsjRawColumnResult``,
        d_offsets, d_valid, d_bytes) -- blocking for the 48-byte result; with sync=False the device tensor that holds it,
        nothing waited for."""
        _check_records(d_rows, "the records")
        capacity, d_offsets, d_valid = self._column_rows(d_rows, d_offsets, d_valid, capacity)
        d_result = self._result(d_result)
        flags = _lib.RAW_COMPACT if compact else 0

        def call(room, d_out):
            rc = self.lib.msj_raw_column_device(self.ctx, _ptr(d_buf), int(length), _ptr(d_idx), int(n), _ptr(d_type), _opt(d_match), _ptr(d_end),
                                                _ptr(d_flags), _ptr(d_rows), _ptr(d_rows_select), _ptr(d_offsets), _ptr(d_valid), capacity,
                                                _opt(d_out), room, flags, _ptr(d_result), self._stream())
            if rc != 0:
                raise RuntimeError(f"msj_raw_column_device failed: {rc}")

        res, (d_bytes,) = self._sized_call(call, _lib.MsjRawColumnResult, d_result, "total_bytes", text, (d_bytes,), bytes_capacity, 1, sync)
        return res, d_offsets, d_valid, d_bytes

    def dictionary(self, d_offsets, d_bytes, d_valid, rows=None, d_n_rows=None, bytes_len=None, d_codes=None, d_dict_offsets=None,
                   d_dict_first=None, d_dict_bytes=None, dict_capacity=None, dict_bytes_capacity=None, values=True, weak_hash=False,
                   d_result=None, sync=True):
        """A byte column as codes plus distinct values (``msj_dictionary_device``), all on the device.  d_offsets (int64,
        rows + 1 entries), d_bytes (uint8) and d_valid (uint8, one per row): what ``string_column`` or ``raw_column`` wrote, or
        any arrays of that shape; rows: default the room of d_offsets; d_n_rows: an int64 device tensor whose first word is
        the number of rows, read on the device (for example the ``n_rows`` of a column call's result tensor: ``d_res[8:16]
        .view(torch.int64)``); bytes_len: default the size of d_bytes.  d_codes: int32 tensor of `rows` entries (default: a
        new one).  d_dict_offsets (int64, dict_capacity + 1), d_dict_first (int32, dict_capacity), d_dict_bytes (uint8,
        dict_bytes_capacity): the caller's, all three or none; without them new ones of the named capacities are made, and
        without those numbers either they are sized from a layout-only first call, whose 48-byte result is waited for.
        values=False: the layout-only form alone (codes and counts; the three are None).  weak_hash: the test aid
        MSJ_DICTIONARY_WEAK_HASH.  Returns (``MsjDictionaryResult``, d_codes, d_dict_offsets, d_dict_first, d_dict_bytes) --
        blocking for the 48-byte result; with sync=False the device tensor that holds it, nothing waited for."""
        rows = d_offsets.numel() - 1 if rows is None else int(rows)
        bytes_len = d_bytes.numel() if bytes_len is None else int(bytes_len)
        if d_codes is None:
            d_codes = torch.empty(max(rows, 1), dtype=torch.int32, device=self.device)
        d_result = self._result(d_result)
        flags = _lib.DICTIONARY_WEAK_HASH if weak_hash else 0

        def call(capacity, room, d_off, d_first, d_out):
            rc = self.lib.msj_dictionary_device(self.ctx, _ptr(d_offsets), _ptr(d_valid), rows, _opt(d_n_rows), _ptr(d_bytes), bytes_len,
                                                _ptr(d_codes), _opt(d_off), _opt(d_first), int(capacity), _opt(d_out), int(room), flags,
                                                _ptr(d_result), self._stream())
            if rc != 0:
                raise RuntimeError(f"msj_dictionary_device failed: {rc}")

        def read():
            return _lib.MsjDictionaryResult.from_buffer_copy(d_result.cpu().numpy().tobytes())

        mine = (d_dict_offsets, d_dict_first, d_dict_bytes)
        if any(t is None for t in mine) != all(t is None for t in mine):
            raise ValueError("d_dict_offsets, d_dict_first and d_dict_bytes: all three or none")
        if not values:
            d_dict_offsets = d_dict_first = d_dict_bytes = None
            dict_capacity = dict_bytes_capacity = 0
        elif d_dict_offsets is None:
            if dict_capacity is None or dict_bytes_capacity is None:
                call(0, 0, None, None, None)
                first = read()
                dict_capacity = first.n_distinct if dict_capacity is None else dict_capacity
                dict_bytes_capacity = first.dict_bytes if dict_bytes_capacity is None else dict_bytes_capacity
            dict_capacity, dict_bytes_capacity = int(dict_capacity), int(dict_bytes_capacity)
            d_dict_offsets = torch.empty(dict_capacity + 1, dtype=torch.int64, device=self.device)
            d_dict_first = torch.empty(max(dict_capacity, 1), dtype=torch.int32, device=self.device)
            d_dict_bytes = torch.empty(max(dict_bytes_capacity, 1), dtype=torch.uint8, device=self.device)
        else:
            if dict_capacity is None:
                dict_capacity = min(d_dict_offsets.numel() - 1, d_dict_first.numel())
            if dict_bytes_capacity is None:
                dict_bytes_capacity = d_dict_bytes.numel()
        call(dict_capacity, dict_bytes_capacity, d_dict_offsets, d_dict_first, d_dict_bytes)
        return (read() if sync else d_result), d_codes, d_dict_offsets, d_dict_first, d_dict_bytes

    def dictionary_extend(self, d_offsets, d_bytes, d_valid, d_dict_offsets=None, d_dict_first=None, d_dict_bytes=None, n_prior=0,
                          d_n_prior=None, rows=None, d_n_rows=None, bytes_len=None, d_codes=None, dict_capacity=None,
                          dict_bytes_capacity=None, frozen=False, weak_hash=False, d_result=None, sync=True):
        """A byte column encoded against the entries the dictionary arrays hold already (``msj_dictionary_extend_device``): a
        prior value keeps its code, a new one is appended behind the n_prior entries -- or, frozen=True, gets code -2 and
        nothing is written to the three arrays.  The column, rows, d_n_rows, bytes_len and d_codes are ``dictionary``'s.
        d_dict_offsets (int64, dict_capacity + 1), d_dict_first (int32, dict_capacity), d_dict_bytes (uint8,
        dict_bytes_capacity): the caller's, as an earlier call of either dictionary call left them (a ``RunningDictionary``
        of ``document_stream`` owns such three), all three or none; none is the layout-only form (codes and counts,
        n_prior 0).  n_prior: the entries they hold; d_n_prior: an int64 device tensor whose first word is that number,
        read on the device (the ``n_distinct`` of the previous call's result tensor: ``d_res[24:32].view(torch.int64)``), so
        that window follows window with nothing waited for.  weak_hash: the test aid.  Returns
        (``MsjDictionaryExtendResult``, d_codes, d_dict_offsets, d_dict_first, d_dict_bytes) -- blocking for the 64-byte
        result; with sync=False the device tensor that holds it, nothing waited for."""
        rows = d_offsets.numel() - 1 if rows is None else int(rows)
        bytes_len = d_bytes.numel() if bytes_len is None else int(bytes_len)
        if d_codes is None:
            d_codes = torch.empty(max(rows, 1), dtype=torch.int32, device=self.device)
        if d_result is None:
            d_result = torch.zeros(64, dtype=torch.uint8, device=self.device)
        mine = (d_dict_offsets, d_dict_first, d_dict_bytes)
        if any(t is None for t in mine) != all(t is None for t in mine):
            raise ValueError("d_dict_offsets, d_dict_first and d_dict_bytes: all three or none")
        if d_dict_offsets is None:
            dict_capacity = dict_bytes_capacity = 0
        else:
            if dict_capacity is None:
                dict_capacity = min(d_dict_offsets.numel() - 1, d_dict_first.numel())
            if dict_bytes_capacity is None:
                dict_bytes_capacity = d_dict_bytes.numel()
        flags = (_lib.DICTIONARY_WEAK_HASH if weak_hash else 0) | (_lib.DICTIONARY_FROZEN if frozen else 0)
        rc = self.lib.msj_dictionary_extend_device(self.ctx, _ptr(d_offsets), _ptr(d_valid), rows, _opt(d_n_rows), _ptr(d_bytes), bytes_len,
                                                   int(n_prior), _opt(d_n_prior), _ptr(d_codes), _opt(d_dict_offsets), _opt(d_dict_first),
                                                   int(dict_capacity), _opt(d_dict_bytes), int(dict_bytes_capacity), flags,
                                                   _ptr(d_result), self._stream())
        if rc != 0:
            raise RuntimeError(f"msj_dictionary_extend_device failed: {rc}")
        res = _lib.MsjDictionaryExtendResult.from_buffer_copy(d_result.cpu().numpy().tobytes()) if sync else d_result
        return res, d_codes, d_dict_offsets, d_dict_first, d_dict_bytes

    def compile_predicates(self, specs, any=False):
        """Compile 1 to 16 row predicates for ``filter_rows`` (``msj_predicates_create``).  A spec is a tuple (column, op,
        operand): ``(0, "==", "error")``, ``(0, "prefix", b"err")``, ``(1, ">", 250)``, ``(1, "<=", 0.5)``, ``(2, "type",
        "object")`` (or a list of "object" "array" "string" "int" "double" "number" "true" "false" "bool" "null"), ``(0,
        "found")``, or ``("not", spec)``.  column: 0..15, the column of the records the call is given.  A str (UTF-8) or
        bytes operand picks the string ops == and prefix; an int (an int64) or a float (finite) the numeric ops == < <= > >=,
        which compare as real numbers, exactly; a bool is rejected.  "not" inverts the truth value also for a row without a
        value.  any=True: a row is kept when any predicate holds (default: all).  The handle is immutable, usable by any
        number of calls, and closed with the device.  ValueError for what is no predicate or beyond the limits."""
        specs = list(specs)
        alive = []
        table = (_lib.MsjPredicate * max(len(specs), 1))(*[predicate_struct(s, alive) for s in specs])
        h = ctypes.c_void_p()
        rc = self.lib.msj_predicates_create(self.ctx, table, len(specs), _lib.PREDICATES_ANY if any else 0, ctypes.byref(h))
        if rc == -1:
            raise ValueError(f"1 to {_lib.MAX_PREDICATES} predicates on columns 0..{_lib.MAX_COLUMNS - 1}, operands of at most "
                             f"{_lib.MAX_OPERAND_BYTES} bytes or finite: {specs}")
        if rc != 0:
            raise RuntimeError(f"msj_predicates_create failed: {rc}")
        predicates = Predicates(self.lib, h, len(specs), max(int(t.column) for t in table), bool(any))
        self._paths.append(predicates)
        return predicates

    @staticmethod
    def _record_columns(d_fields, what):
        """Records as int64 of shape (rows, 2) or (n_columns, rows, 2) -> (n_columns, rows, stride in records)"""
        if d_fields.dim() == 2:
            _check_records(d_fields, what)
            return 1, d_fields.shape[0], d_fields.shape[0]
        _check_records(d_fields[0], what)
        stride = d_fields.stride(0) // 2 if d_fields.shape[0] > 1 else d_fields.shape[1]
        if d_fields.shape[0] > 1 and d_fields.stride(0) % 2:
            raise ValueError(f"{what} must be contiguous")
        return d_fields.shape[0], d_fields.shape[1], stride

    def filter_rows(self, predicates, d_buf, length, d_fields, d_rows_select, capacity=None, d_keep=None, d_kept=None, kept=True,
                    d_list_offsets=None, list_rows=None, d_list_n_rows=None, d_list_offsets_out=None, d_result=None, d_kept_select=None,
                    sync=True):
        """Rows by predicate (``msj_filter_rows_device``): a keep byte per row and the kept row numbers ascending, all on
        the device.  predicates: from ``compile_predicates``; d_buf / length: the window the records were written over;
        d_fields: int64 of shape (n_columns, rows, 2) -- what ``select_documents`` or ``select_elements`` wrote -- or (rows, 2)
        for a single column; d_rows_select: the device ``msj_select_documents_result`` that counts the rows, read on the
        device.  capacity: default the rows of d_fields.  d_keep: uint8 tensor of capacity entries, d_kept: int32 tensor of
        capacity entries (default: new ones); kept=False: the mask-only form (d_kept None).  d_list_offsets: int64 tensor,
        the offsets of a list column whose elements are these rows, list_rows + 1 entries (default: its room), d_list_n_rows
        an int64 device word that holds the list's rows; d_list_offsets_out receives the re-based offsets (default: a new
        one).  d_kept_select: uint8[48] that receives the ``msj_select_documents_result`` that counts the kept rows (default:
        a new one) -- what ``take_rows`` reads as d_take_select.  Returns (``MsjFilterRowsResult``, d_keep, d_kept,
        d_kept_select, d_list_offsets_out) -- blocking for the 48-byte result; with sync=False the device tensor that holds
        it, nothing waited for."""
        n_columns, rows, stride = self._record_columns(d_fields, "the records")
        capacity = rows if capacity is None else int(capacity)
        if d_keep is None:
            d_keep = torch.empty(max(capacity, 1), dtype=torch.uint8, device=self.device)
        if not kept:
            d_kept = None
        elif d_kept is None:
            d_kept = torch.empty(max(capacity, 1), dtype=torch.int32, device=self.device)
        if d_list_offsets is not None:
            list_rows = d_list_offsets.numel() - 1 if list_rows is None else int(list_rows)
            if d_list_offsets_out is None:
                d_list_offsets_out = torch.empty(list_rows + 1, dtype=torch.int64, device=self.device)
        d_result, d_kept_select = self._result(d_result), self._result(d_kept_select)
        rc = self.lib.msj_filter_rows_device(
            self.ctx, predicates.handle, _ptr(d_buf), int(length), _ptr(d_fields), stride, n_columns, _ptr(d_rows_select), _ptr(d_keep),
            _opt(d_kept), capacity, _opt(d_list_offsets), int(list_rows or 0), _opt(d_list_n_rows), _opt(d_list_offsets_out), _ptr(d_result),
            _ptr(d_kept_select), self._stream())
        if rc != 0:
            raise RuntimeError(f"msj_filter_rows_device failed: {rc}")
        res = _lib.MsjFilterRowsResult.from_buffer_copy(d_result.cpu().numpy().tobytes()) if sync else d_result
        return res, d_keep, d_kept, d_kept_select, d_list_offsets_out

    def take_rows(self, d_take, d_take_select, d_fields, d_rows_select, d_out=None, out_capacity=None, d_result=None, d_out_select=None,
                  sync=True):
        """Records gathered by a selection vector (``msj_take_rows_device``): d_out[c, j] = d_fields[c, d_take[j]], all on
        the device.  d_take: int32 tensor of row numbers, any order, repeats allowed -- ``filter_rows``' d_kept, ``dictionary``'s
        d_dict_first; d_take_select: the device ``msj_select_documents_result`` whose n_documents counts them
        (``filter_rows``' d_kept_select), read on the device; d_fields / d_rows_select: the records, int64 of shape
        (n_columns, rows, 2) or (rows, 2), and the select result that counts their rows.  An index at or past the rows gives
        the record of a missing value.  d_out: int64 tensor of shape (n_columns, out_capacity, 2) (default: a new one,
        out_capacity = the entries of d_take).  d_out_select: uint8[48] that receives the ``msj_select_documents_result`` of
        d_out (default: a new one), so that every call that takes records takes these.  Returns (``MsjTakeRowsResult``, d_out,
        d_out_select) -- blocking for the 48-byte result; with sync=False the device tensor that holds it, nothing waited
        for."""
        n_columns, _, stride = self._record_columns(d_fields, "the records")
        if d_out is None:
            out_capacity = d_take.numel() if out_capacity is None else int(out_capacity)
            d_out = torch.empty((n_columns, max(out_capacity, 1), 2), dtype=torch.int64, device=self.device)
        out_columns, out_rows, out_stride = self._record_columns(d_out, "the output records")
        if out_columns != n_columns:
            raise ValueError("d_out has as many columns as d_fields")
        out_capacity = out_rows if out_capacity is None else int(out_capacity)
        d_result, d_out_select = self._result(d_result), self._result(d_out_select)
        rc = self.lib.msj_take_rows_device(self.ctx, _ptr(d_take), _ptr(d_take_select), _ptr(d_fields), stride, n_columns, _ptr(d_rows_select),
                                           _ptr(d_out), out_stride, out_capacity, _ptr(d_result), _ptr(d_out_select), self._stream())
        if rc != 0:
            raise RuntimeError(f"msj_take_rows_device failed: {rc}")
        res = _lib.MsjTakeRowsResult.from_buffer_copy(d_result.cpu().numpy().tobytes()) if sync else d_result
        return res, d_out, d_out_select

    def cast_strings(self, d_window, length, d_rows, d_rows_select, kind, unit="ns", keep_numbers=False, capacity=None, d_out=None,
                     d_result=None, d_out_select=None, sync=True):
        """Timestamps and numbers written as strings, as number records (``msj_cast_strings_device``), all on the device.
        d_window / length: the window the records were written over; d_rows: int64 of shape (rows, 2), any ``msj_field``
        records -- a path of ``select_documents`` or ``select_elements``, the elements of a list column, taken rows;
        d_rows_select: the device ``msj_select_documents_result`` that counts them, read on the device.  kind: "timestamp"
        (RFC 3339; the int64 counts `unit` -- "s" "ms" "us" "ns" -- since 1970-01-01T00:00:00Z, a fraction cut to the unit)
        or "number" (the string, whole, is one JSON number: an exact int64 or the nearest double; the unit is ignored).
        keep_numbers: a row that already is a number is copied instead of becoming code 17.  capacity: default the rows of
        d_rows.  d_out: int64 tensor of shape (capacity, 2) (default: a new one); d_rows itself casts in place.  d_out_select:
        uint8[48] that receives the ``msj_select_documents_result`` of d_out (default: a new one), so that ``filter_rows``,
        ``take_rows`` and ``number_column`` take the cast records as they take a select call's.  Returns
        (``MsjCastStringsResult``, d_out, d_out_select) -- blocking for the 48-byte result; with sync=False the device tensor
        that holds it, nothing waited for."""
        _check_records(d_rows, "the records")
        if kind not in _lib.CAST_KINDS or unit not in _lib.CAST_UNITS:
            raise ValueError(f"kind is one of {sorted(_lib.CAST_KINDS)}, unit one of {sorted(_lib.CAST_UNITS)}: {kind!r}, {unit!r}")
        capacity = d_rows.shape[0] if capacity is None else int(capacity)
        if d_out is None:
            d_out = torch.empty((max(capacity, 1), 2), dtype=torch.int64, device=self.device)
        _check_records(d_out, "the output records")
        d_result, d_out_select = self._result(d_result), self._result(d_out_select)
        number = kind == "number"
        rc = self.lib.msj_cast_strings_device(self.ctx, _ptr(d_window), int(length), _ptr(d_rows), _ptr(d_rows_select), _lib.CAST_KINDS[kind],
                                              0 if number else _lib.CAST_UNITS[unit], _lib.CAST_KEEP_NUMBERS if keep_numbers else 0,
                                              _ptr(d_out), capacity, _ptr(d_result), _ptr(d_out_select), self._stream())
        if rc != 0:
            raise RuntimeError(f"msj_cast_strings_device failed: {rc}")
        res = _lib.MsjCastStringsResult.from_buffer_copy(d_result.cpu().numpy().tobytes()) if sync else d_result
        return res, d_out, d_out_select

    def bucket_rows(self, d_rows, d_rows_select, width, origin=0, capacity=None, d_out=None, d_result=None, d_out_select=None, sync=True):
        """Numbers floored to multiples of a width (``msj_bucket_rows_device``), all on the device: the record of a number
        value becomes the int64 ``origin + floor((floor(v) - origin) / width) * width``, exactly -- a timestamp cast to
        milliseconds with width 60 000 is its minute, also before 1970.  d_rows: int64 of shape (rows, 2), any ``msj_field``
        records -- a path of ``select_documents``, cast strings, taken rows; d_rows_select: the device
        ``msj_select_documents_result`` that counts them, read on the device.  width: an int of at least 1; origin: an int.
        A record with a code is copied; a number whose bucket leaves int64 and a number without bits become code 9, anything
        else code 17.  capacity: default the rows of d_rows.  d_out: int64 tensor of shape (capacity, 2) (default: a new one);
        d_rows itself buckets in place.  d_out_select: uint8[48] that receives the ``msj_select_documents_result`` of d_out
        (default: a new one).  Returns (``MsjBucketRowsResult``, d_out, d_out_select) -- blocking for the 48-byte result;
        with sync=False the device tensor that holds it, nothing waited for."""
        _check_records(d_rows, "the records")
        width, origin = int(width), int(origin)
        if width < 1 or width >= 1 << 63 or not -(1 << 63) <= origin < 1 << 63:
            raise ValueError(f"width lies in 1..2^63 - 1 and origin in int64: {width!r}, {origin!r}")
        capacity = d_rows.shape[0] if capacity is None else int(capacity)
        if d_out is None:
            d_out = torch.empty((max(capacity, 1), 2), dtype=torch.int64, device=self.device)
        _check_records(d_out, "the output records")
        d_result, d_out_select = self._result(d_result), self._result(d_out_select)
        rc = self.lib.msj_bucket_rows_device(self.ctx, _ptr(d_rows), _ptr(d_rows_select), width, origin, 0, _ptr(d_out), capacity,
                                             _ptr(d_result), _ptr(d_out_select), self._stream())
        if rc != 0:
            raise RuntimeError(f"msj_bucket_rows_device failed: {rc}")
        res = _lib.MsjBucketRowsResult.from_buffer_copy(d_result.cpu().numpy().tobytes()) if sync else d_result
        return res, d_out, d_out_select

    def group_keys(self, parts, d_rows_select, capacity=None, d_offsets=None, d_valid=None, d_bytes=None, d_result=None, sync=True):
        """One fixed-width, order-preserving byte key per row from 1 to 8 columns (``msj_group_keys_device``), all on the
        device, in the (d_offsets, d_valid, d_bytes) layout ``dictionary`` and ``dictionary_extend`` take: their codes are the
        rows' groups.  parts: a list of tensors or of (tensor, null_is_group) pairs -- int64 of shape (rows, 2) is a NUMBER
        part (``msj_field`` records: 11 key bytes; equal reals have equal bytes and the bytes order as the reals do), int32
        of `rows` entries a CODE part (5 key bytes; a code below 0 is null).  Every part has the same rows.  A row with a null
        part has no key (d_valid 0) unless that part says null_is_group.  d_rows_select: the device
        ``msj_select_documents_result`` that counts the rows, read on the device.  capacity: default the rows of the parts.
        d_offsets (int64, capacity + 1), d_valid (uint8, capacity), d_bytes (uint8, capacity * W, 16-byte aligned): the
        caller's or new ones.  Returns (``MsjGroupKeysResult``, d_offsets, d_valid, d_bytes) -- blocking for the 48-byte
        result; with sync=False the device tensor that holds it, nothing waited for."""
        parts = [p if isinstance(p, (tuple, list)) else (p, False) for p in parts]
        if not 1 <= len(parts) <= _lib.KEY_MAX_PARTS:
            raise ValueError(f"1 to {_lib.KEY_MAX_PARTS} parts: {len(parts)}")
        table = (_lib.MsjKeyPart * len(parts))()
        stride, W = None, 0
        for j, (t, null_is_group) in enumerate(parts):
            if t.dtype == torch.int64:
                _check_records(t, "a NUMBER part")
                kind, rows = _lib.KEY_NUMBER, t.shape[0]
            elif t.dtype == torch.int32 and t.dim() == 1 and t.stride(-1) == 1:
                kind, rows = _lib.KEY_CODE, t.numel()
            else:
                raise ValueError("a part is int64 records of shape (rows, 2) or a contiguous int32 tensor of codes")
            if stride is not None and rows != stride:
                raise ValueError("every part has the same rows")
            stride = rows
            table[j].d_column, table[j].kind, table[j].flags = t.data_ptr(), kind, _lib.KEY_NULL_IS_GROUP if null_is_group else 0
            W += _lib.KEY_PART_BYTES[kind]
        capacity = stride if capacity is None else int(capacity)
        capacity, d_offsets, d_valid = self._column_rows(parts[0][0], d_offsets, d_valid, capacity)
        bytes_capacity = capacity * W if d_bytes is None else d_bytes.numel()
        if d_bytes is None:
            d_bytes = torch.empty(max(bytes_capacity, 1), dtype=torch.uint8, device=self.device)
        d_result = self._result(d_result)
        rc = self.lib.msj_group_keys_device(self.ctx, table, len(parts), stride, _ptr(d_rows_select), _ptr(d_offsets), _ptr(d_valid), _ptr(d_bytes),
                                            capacity, bytes_capacity, _ptr(d_result), self._stream())
        if rc != 0:
            raise RuntimeError(f"msj_group_keys_device failed: {rc}")
        res = _lib.MsjGroupKeysResult.from_buffer_copy(d_result.cpu().numpy().tobytes()) if sync else d_result
        return res, d_offsets, d_valid, d_bytes

    def aggregate(self, d_fields, d_rows_select, d_codes=None, n_groups=1, d_n_groups=None, d_groups=None, groups_capacity=None,
                  d_result=None, sync=True):
        """Count, sum, min and max per group (``msj_aggregate_device``), exact and bit for bit the same from run to run, all
        on the device.  d_fields: int64 of shape (n_columns, rows, 2) or (rows, 2), any ``msj_field`` records -- paths of
        ``select_documents`` or ``select_elements``, cast strings, taken rows; d_rows_select: the device
        ``msj_select_documents_result`` that counts the rows, read on the device.  d_codes: int32 tensor, a group per row --
        ``dictionary``'s d_codes, or any codes; a row whose code lies outside [0, G) is in no group; None: every row is
        group 0.  G is n_groups, or with d_n_groups an int64 device word read on the device (the ``n_distinct`` of a
        dictionary's result tensor: ``d_res[24:32].view(torch.int64)``).  d_groups: uint8 tensor of n_columns *
        groups_capacity * 48 bytes that receives the ``msj_aggregate`` records, column c's at c * groups_capacity (default: a
        new one; groups_capacity: default n_groups).  Returns (``MsjAggregateResult``, d_groups) -- blocking for the 48-byte
        result; with sync=False the device tensor that holds it, nothing waited for."""
        n_columns, rows, stride = self._record_columns(d_fields, "the records")
        if d_codes is not None and (d_codes.dtype != torch.int32 or d_codes.stride(-1) != 1 or d_codes.numel() < stride):
            raise ValueError("d_codes is a contiguous int32 tensor with an entry per row of d_fields")
        if groups_capacity is None:
            groups_capacity = int(n_groups) if d_groups is None else d_groups.numel() // (48 * n_columns)
        groups_capacity = int(groups_capacity)
        if d_groups is None:
            d_groups = torch.empty(max(n_columns * groups_capacity, 1) * 48, dtype=torch.uint8, device=self.device)
        if d_groups.dtype != torch.uint8 or d_groups.numel() < n_columns * groups_capacity * 48:
            raise ValueError("d_groups is a uint8 tensor of n_columns * groups_capacity * 48 bytes")
        d_result = self._result(d_result)
        rc = self.lib.msj_aggregate_device(self.ctx, _ptr(d_fields), stride, n_columns, _ptr(d_rows_select), _opt(d_codes), int(n_groups),
                                           _opt(d_n_groups), _ptr(d_groups), groups_capacity, _ptr(d_result), self._stream())
        if rc != 0:
            raise RuntimeError(f"msj_aggregate_device failed: {rc}")
        res = _lib.MsjAggregateResult.from_buffer_copy(d_result.cpu().numpy().tobytes()) if sync else d_result
        return res, d_groups

    def set_aggregate_limits(self, lds_groups=_lib.AGG_MAX_LDS_GROUPS):
        """Test hook: the most groups ``aggregate`` sums in LDS (0: never; default and most: 256).  The records do not
        change."""
        if self.lib.msj_debug_set_aggregate_limits(self.ctx, int(lds_groups)) != 0:
            raise ValueError(f"lds_groups lies in 0..{_lib.AGG_MAX_LDS_GROUPS}: {lds_groups!r}")

    def sort_rows(self, d_fields, d_rows_select, d_rows_in=None, d_rows_in_select=None, descending=False, values_only=False, limit=0,
                  capacity=None, d_order=None, d_result=None, d_order_select=None, sync=True):
        """Row numbers in the exact numeric order of one column's values (``msj_sort_rows_device``), stable, all on the
        device.  d_fields: int64 of shape (rows, 2), ONE column of ``msj_field`` records -- a path of ``select_documents``,
        cast strings, taken rows; d_rows_select: the device ``msj_select_documents_result`` that counts its rows, read on
        the device.  d_rows_in / d_rows_in_select: an int32 tensor of row numbers to order instead of all the rows, in any
        order, repeats allowed, with the device select result that counts them -- ``filter_rows``' d_kept and
        d_kept_select, or an earlier call's d_order and d_order_select for the major key of a two-key sort (the sort is
        stable).  An int64 is compared with a double as real numbers; equal values keep the input order; rows without a
        number value come last in input order, or are left out with values_only.  descending reverses the values' order
        only.  limit: only the first so many row numbers are written (0: all).  capacity: the most input rows (default:
        the entries of d_rows_in, or the rows of d_fields).  d_order: int32 tensor of capacity entries -- min(capacity,
        limit) with a limit -- (default: a new one); d_order_select: uint8[48] that receives the
        ``msj_select_documents_result`` counting the entries written (default: a new one): the pair is what ``take_rows``
        takes as d_take / d_take_select.  Returns (``MsjSortRowsResult``, d_order, d_order_select) -- blocking for the
        48-byte result; with sync=False the device tensor that holds it, nothing waited for."""
        _check_records(d_fields, "the records")
        if (d_rows_in is None) != (d_rows_in_select is None):
            raise ValueError("d_rows_in and d_rows_in_select come together")
        if d_rows_in is not None and (d_rows_in.dtype != torch.int32 or d_rows_in.stride(-1) != 1):
            raise ValueError("d_rows_in is a contiguous int32 tensor")
        stride = d_fields.shape[0]
        if capacity is None:
            capacity = d_rows_in.numel() if d_rows_in is not None else stride
        capacity, limit = int(capacity), int(limit)
        room = min(capacity, limit) if limit > 0 else capacity
        if d_order is None:
            d_order = torch.empty((max(room, 1),), dtype=torch.int32, device=self.device)
        if d_order.dtype != torch.int32 or d_order.numel() < room or (d_rows_in is not None and d_rows_in.numel() < capacity):
            raise ValueError("d_order is an int32 tensor with room for the rows written, d_rows_in has capacity entries")
        d_result, d_order_select = self._result(d_result), self._result(d_order_select)
        flags = (_lib.SORT_DESCENDING if descending else 0) | (_lib.SORT_VALUES_ONLY if values_only else 0)
        rc = self.lib.msj_sort_rows_device(self.ctx, _ptr(d_fields), stride, _ptr(d_rows_select), _opt(d_rows_in), _opt(d_rows_in_select), flags,
                                           limit, _ptr(d_order), capacity, _ptr(d_result), _ptr(d_order_select), self._stream())
        if rc != 0:
            raise RuntimeError(f"msj_sort_rows_device failed: {rc}")
        res = _lib.MsjSortRowsResult.from_buffer_copy(d_result.cpu().numpy().tobytes()) if sync else d_result
        return res, d_order, d_order_select

    def join_rows(self, d_left_keys, d_right_keys, n_keys=0, d_n_keys=None, keys_capacity=None, how="inner", left_rows=None, d_n_left=None,
                  right_rows=None, d_n_right=None, pairs_capacity=None, d_left_rows=None, d_right_rows=None, right=True, d_offsets=None,
                  offsets=False, d_result=None, d_left_select=None, d_right_select=None, sync=True):
        """The equi-join of two int32 code columns as row pairs (``msj_join_rows_device``), all on the device.
        d_left_keys / d_right_keys: contiguous int32 tensors, codes of ONE dictionary (``dictionary_extend`` over both
        sides); left_rows / right_rows: their rows (default: their entries), which are also the rooms; d_n_left / d_n_right
        / d_n_keys: int64 device tensors whose first word is L, R or G, read on the device -- ``d_res[8:16]`` of a
        dictionary call's result is its n_rows, ``d_res[24:32]`` its n_distinct -- so a join follows two dictionary calls
        with nothing waited for; n_keys: G otherwise; keys_capacity: the most G can be (default: n_keys).  A code outside
        [0, G) -- -1, -2 -- equals nothing.  how: "inner", "left" (a left row without a partner is paired with
        ``JOIN_NO_ROW``), "semi" (each left row with a partner once, with its first), "anti" (each left row without one).
        Pairs come in ascending left row and, inside one, ascending right row.  pairs_capacity: the room of the pair
        tensors (default: their entries, or the left rows); d_left_rows / d_right_rows: int32 tensors (default: new ones;
        right=False: no right tensor, nothing written for it); d_offsets: int64 tensor of left_rows + 1 entries, or
        offsets=True for a new one: the pairs in front of every left row, a list column over the left rows.
        d_left_select / d_right_select: uint8[48] tensors that receive the ``msj_select_documents_result`` counting the
        pairs -- with a pair tensor what ``take_rows`` takes as d_take / d_take_select.  A result with code 1
        (MSJ_CAPACITY) and n_pairs above the room: nothing was written to the pair tensors; repeat with n_pairs entries.
        Returns (``MsjJoinRowsResult``, d_left_rows, d_right_rows, d_offsets, d_left_select, d_right_select) -- blocking
        for the 64-byte result; with sync=False the device tensor that holds it, nothing waited for."""
        for t in (d_left_keys, d_right_keys):
            if t.dtype != torch.int32 or t.stride(-1) != 1:
                raise ValueError("the keys are contiguous int32 tensors")
        if how not in _lib.JOIN_KINDS:
            raise ValueError(f"how is one of {sorted(_lib.JOIN_KINDS)}: {how!r}")
        left_rows = d_left_keys.numel() if left_rows is None else int(left_rows)
        right_rows = d_right_keys.numel() if right_rows is None else int(right_rows)
        keys_capacity = int(n_keys) if keys_capacity is None else int(keys_capacity)
        if pairs_capacity is None:
            pairs_capacity = d_left_rows.numel() if d_left_rows is not None else left_rows
        pairs_capacity = int(pairs_capacity)
        if d_left_rows is None:
            d_left_rows = torch.empty((max(pairs_capacity, 1),), dtype=torch.int32, device=self.device)
        if d_right_rows is None and right:
            d_right_rows = torch.empty((max(pairs_capacity, 1),), dtype=torch.int32, device=self.device)
        if d_offsets is None and offsets:
            d_offsets = torch.empty((left_rows + 1,), dtype=torch.int64, device=self.device)
        for t in (d_left_rows, d_right_rows):
            if t is not None and (t.dtype != torch.int32 or t.numel() < pairs_capacity):
                raise ValueError("the pair tensors are int32 with pairs_capacity entries")
        if d_offsets is not None and (d_offsets.dtype != torch.int64 or d_offsets.numel() < left_rows + 1):
            raise ValueError("d_offsets is an int64 tensor of left_rows + 1 entries")
        if d_result is None:
            d_result = torch.zeros(64, dtype=torch.uint8, device=self.device)
        d_left_select, d_right_select = self._result(d_left_select), self._result(d_right_select)
        rc = self.lib.msj_join_rows_device(self.ctx, _ptr(d_left_keys), left_rows, _opt(d_n_left), _ptr(d_right_keys), right_rows, _opt(d_n_right),
                                           int(n_keys), _opt(d_n_keys), keys_capacity, _lib.JOIN_KINDS[how], _ptr(d_left_rows), _opt(d_right_rows),
                                           pairs_capacity, _opt(d_offsets), _ptr(d_result), _ptr(d_left_select), _ptr(d_right_select),
                                           self._stream())
        if rc != 0:
            raise RuntimeError(f"msj_join_rows_device failed: {rc}")
        res = _lib.MsjJoinRowsResult.from_buffer_copy(d_result.cpu().numpy().tobytes()) if sync else d_result
        return res, d_left_rows, d_right_rows, d_offsets, d_left_select, d_right_select

    def join_rows_workspace_bytes(self, left_rows, right_rows, keys_capacity):
        """The device workspace one ``join_rows`` call of these rooms keeps in the context (``msj_join_rows_workspace_bytes``)."""
        return int(self.lib.msj_join_rows_workspace_bytes(int(left_rows), int(right_rows), int(keys_capacity)))

    def dictionary_order(self, d_dict_offsets, d_dict_bytes, n_entries=0, d_n_entries=None, capacity=None, dict_bytes_capacity=None, depth=0,
                         max_rounds=0, resume=False, d_sorted=None, d_rank=None, d_result=None, sync=True):
        """A dictionary's entries in the byte order of their values (``msj_dictionary_order_device``), all on the device.
        d_dict_offsets (int64, capacity + 1 entries) and d_dict_bytes (uint8): what ``dictionary`` / ``dictionary_extend``
        wrote, or any arrays of that shape; n_entries: V; d_n_entries: an int64 device tensor whose first word is V, read on
        the device (``d_res[24:32].view(torch.int64)`` of a dictionary call's result is its n_distinct); capacity: the room
        of d_sorted / d_rank (default: the room of d_dict_offsets); dict_bytes_capacity: default the size of d_dict_bytes.
        Values compare as unsigned bytes, a proper prefix first.  d_sorted / d_rank: int32 tensors of `capacity` entries
        (default: new ones) -- the entry numbers in order, and per entry the number of smaller values (``ORDER_NO_RANK``,
        as int32 -1, for an entry without a value).  max_rounds: the rounds of eight bytes this call may compare (0: the
        path's default).  A result with code 1 (MSJ_CAPACITY) and n_tied > 0: entries still agree on `depth` bytes; repeat
        with resume=True, depth=result.depth and the same two tensors.  Returns (``MsjDictionaryOrderResult``, d_sorted,
        d_rank) -- blocking for the 48-byte result; with sync=False the device tensor that holds it, nothing waited for."""
        if d_dict_offsets.dtype != torch.int64 or d_dict_offsets.stride(-1) != 1 or d_dict_bytes.dtype != torch.uint8:
            raise ValueError("the dictionary is a contiguous int64 offsets tensor and a uint8 bytes tensor")
        capacity = max(d_dict_offsets.numel() - 1, 0) if capacity is None else int(capacity)
        if d_dict_offsets.numel() < capacity + 1 and capacity > 0:
            raise ValueError("d_dict_offsets has capacity + 1 entries")
        dict_bytes_capacity = d_dict_bytes.numel() if dict_bytes_capacity is None else int(dict_bytes_capacity)
        if d_sorted is None:
            d_sorted = torch.empty((max(capacity, 1),), dtype=torch.int32, device=self.device)
        if d_rank is None:
            d_rank = torch.empty((max(capacity, 1),), dtype=torch.int32, device=self.device)
        for t in (d_sorted, d_rank):
            if t.dtype != torch.int32 or t.numel() < capacity:
                raise ValueError("d_sorted and d_rank are int32 tensors of capacity entries")
        d_result = self._result(d_result)
        rc = self.lib.msj_dictionary_order_device(self.ctx, _ptr(d_dict_offsets), _ptr(d_dict_bytes), dict_bytes_capacity, int(n_entries),
                                                  _opt(d_n_entries), capacity, int(depth), int(max_rounds), _lib.ORDER_CONTINUE if resume else 0,
                                                  _ptr(d_sorted), _ptr(d_rank), _ptr(d_result), self._stream())
        if rc != 0:
            raise RuntimeError(f"msj_dictionary_order_device failed: {rc}")
        res = _lib.MsjDictionaryOrderResult.from_buffer_copy(d_result.cpu().numpy().tobytes()) if sync else d_result
        return res, d_sorted, d_rank

    def dictionary_order_workspace_bytes(self, capacity):
        """The device workspace one ``dictionary_order`` call of this room keeps in the context."""
        return int(self.lib.msj_dictionary_order_workspace_bytes(int(capacity)))

    def set_order_mode(self, mode=_lib.ORDER_MODE_AUTO):
        """Test hook: the path ``dictionary_order`` takes -- 0 by capacity, 1 always the grid path, 2 the one-workgroup path
        wherever capacity <= 1 024.  The order does not change."""
        if self.lib.msj_debug_set_order_mode(self.ctx, int(mode)) != 0:
            raise ValueError(f"mode is 0, 1 or 2: {mode!r}")

    def rank_rows(self, d_codes, d_rank, d_order_result, rows=None, d_n_rows=None, rank_capacity=None, d_fields=None, capacity=None,
                  d_result=None, d_select=None, sync=True):
        """A column of dictionary codes as records that order like the strings (``msj_rank_rows_device``): row k with a
        code that has a rank gets the 'l' record of that rank, every other row (null -1, frozen miss -2, a wild code) the
        record of a missing value.  d_codes: contiguous int32; d_rank and d_order_result: what ``dictionary_order`` wrote
        (the result as the uint8[48] device tensor of its sync=False form); rows: default the entries of d_codes; d_n_rows:
        an int64 device tensor whose first word is R; d_fields: int64 (capacity, 2) (default: a new one).  d_select
        receives the select result over the records, so ``sort_rows``, ``filter_rows``, ``aggregate`` and ``take_rows`` run on
        them.  A code in d_order_result -- an order with entries still tied included -- passes through and nothing is
        written.  Returns (``MsjRankRowsResult``, d_fields, d_select) -- blocking for the 48-byte result; with sync=False
        the device tensor that holds it."""
        if d_codes.dtype != torch.int32 or d_codes.stride(-1) != 1 or d_rank.dtype != torch.int32:
            raise ValueError("the codes and the ranks are contiguous int32 tensors")
        rows = d_codes.numel() if rows is None else int(rows)
        rank_capacity = d_rank.numel() if rank_capacity is None else int(rank_capacity)
        if capacity is None:
            capacity = d_fields.shape[0] if d_fields is not None else rows
        capacity = int(capacity)
        if d_fields is None:
            d_fields = torch.empty((max(capacity, 1), 2), dtype=torch.int64, device=self.device)
        _check_records(d_fields, "d_fields")
        if d_fields.shape[0] < capacity:
            raise ValueError("d_fields has capacity records")
        d_result, d_select = self._result(d_result), self._result(d_select)
        rc = self.lib.msj_rank_rows_device(self.ctx, _ptr(d_codes), rows, _opt(d_n_rows), _ptr(d_rank), rank_capacity, _ptr(d_order_result),
                                           _ptr(d_fields), capacity, _ptr(d_result), _ptr(d_select), self._stream())
        if rc != 0:
            raise RuntimeError(f"msj_rank_rows_device failed: {rc}")
        res = _lib.MsjRankRowsResult.from_buffer_copy(d_result.cpu().numpy().tobytes()) if sync else d_result
        return res, d_fields, d_select

    def compile_patterns(self, specs):
        """Compile 1 to 16 substring patterns for ``match_strings`` (``msj_patterns_create``).  A spec is ``bytes`` or ``str``
        (UTF-8) -- the value contains it --, or ``(pieces, flags)``: 1 to 4 literal pieces of 1 to 255 bytes that must stand
        in the value in this order without overlapping, and a collection of "at_start" (the first piece at the value's first
        byte), "at_end" (the last piece at its end) and "nocase" (A-Z as a-z).  ``([b"GET ", b".png"], {"at_start",
        "at_end"})`` is LIKE 'GET %.png'.  No byte is special.  The handle is immutable, usable by any number of calls, and
        closed with the device.  ValueError for what is no pattern or beyond the limits."""
        specs = list(specs)
        if not 1 <= len(specs) <= _lib.MATCH_MAX_PATTERNS:
            raise ValueError(f"1 to {_lib.MATCH_MAX_PATTERNS} patterns: {len(specs)}")
        alive = []
        table = (_lib.MsjPattern * len(specs))(*[pattern_struct(s, alive) for s in specs])
        h = ctypes.c_void_p()
        rc = self.lib.msj_patterns_create(self.ctx, table, len(specs), 0, ctypes.byref(h))
        if rc == -1:
            raise ValueError(f"no such patterns: {specs}")
        if rc != 0:
            raise RuntimeError(f"msj_patterns_create failed: {rc}")
        patterns = Patterns(self.lib, h, len(specs), max(int(t.n_pieces) for t in table))
        self._paths.append(patterns)
        return patterns

    def match_strings(self, patterns, d_offsets, d_valid, d_bytes, rows=None, d_n_rows=None, bytes_len=None, capacity=None, d_fields=None,
                      d_result=None, d_select=None, sync=True):
        """Substring patterns over a byte column (``msj_match_strings_device``): per (pattern, row) the first place where
        the pattern matches as an 'l' record, or the record of a missing value, all on the device.  patterns: from
        ``compile_patterns``; d_offsets (int64, rows + 1 entries), d_valid (uint8, one per row) and d_bytes (uint8): what
        ``string_column`` or ``raw_column`` wrote, or any arrays of that shape; rows: default the room of d_offsets;
        d_n_rows: an int64 device tensor whose first word is the number of rows, read on the device; bytes_len: default the
        size of d_bytes.  d_fields: int64 (n_patterns, capacity, 2) (default: a new one, capacity = rows).  d_select
        receives the select result over the records, so ``filter_rows`` (``(p, "found")`` is "contains"), ``take_rows``,
        ``aggregate`` and ``sort_rows`` run on them.  Offsets that do not ascend inside bytes_len: code -1 in both results and
        nothing written.  Returns (``MsjMatchStringsResult``, d_fields, d_select) -- blocking for the 48-byte result; with
        sync=False the device tensor that holds it."""
        if d_offsets.dtype != torch.int64 or d_offsets.stride(-1) != 1 or d_valid.dtype != torch.uint8 or d_bytes.dtype != torch.uint8:
            raise ValueError("the offsets are a contiguous int64 tensor, d_valid and d_bytes uint8 tensors")
        rows = d_offsets.numel() - 1 if rows is None else int(rows)
        bytes_len = d_bytes.numel() if bytes_len is None else int(bytes_len)
        if capacity is None:
            capacity = d_fields.shape[1] if d_fields is not None else rows
        capacity = int(capacity)
        if d_fields is None:
            d_fields = torch.empty((patterns.n_patterns, max(capacity, 1), 2), dtype=torch.int64, device=self.device)
        if d_fields.dim() != 3 or d_fields.shape[0] != patterns.n_patterns or not d_fields.is_contiguous() or d_fields.shape[1] != max(capacity, 1):
            raise ValueError("d_fields is a contiguous int64 tensor of shape (n_patterns, capacity, 2)")
        d_result, d_select = self._result(d_result), self._result(d_select)
        rc = self.lib.msj_match_strings_device(self.ctx, patterns.handle, _ptr(d_offsets), _ptr(d_valid), rows, _opt(d_n_rows),
                                               _ptr(d_bytes) if bytes_len else None, bytes_len, _ptr(d_fields), capacity, _ptr(d_result),
                                               _ptr(d_select), self._stream())
        if rc != 0:
            raise RuntimeError(f"msj_match_strings_device failed: {rc}")
        res = _lib.MsjMatchStringsResult.from_buffer_copy(d_result.cpu().numpy().tobytes()) if sync else d_result
        return res, d_fields, d_select

    def set_sort_mode(self, mode=_lib.SORT_MODE_AUTO):
        """Test hook: the path ``sort_rows`` takes -- 0 chosen on the device, 1 always the full sort, 2 always the
        selection.  The order does not change."""
        if self.lib.msj_debug_set_sort_mode(self.ctx, int(mode)) != 0:
            raise ValueError(f"mode is 0, 1 or 2: {mode!r}")

    def array_column(self, d_idx, n, d_type, d_depth, d_match, d_end, d_flags, d_doc_first, d_docs, d_fields, p, d_select_result,
                     d_numbers=None, numbers_capacity=0, d_numbers_result=None, d_offsets=None, d_valid=None, d_elements=None,
                     capacity=None, elements_capacity=None, elements=True, d_result=None, d_elements_select=None, sync=True):
        """One path's arrays as a list column (``msj_array_column_device``): offsets, a validity byte per row and one
        ``msj_field`` per element back to back, all on the device.  The token arrays, the split and the number records with
        their result: those ``select_documents`` ran over; d_fields: its records, int64 of shape (n_paths, rows, 2); p: the
        path's index; d_select_result: the device ``msj_select_documents_result`` of that call.  d_offsets: int64 tensor of
        capacity + 1 entries, d_valid: uint8 tensor of capacity entries (default: new ones, capacity = the rows of d_fields);
        d_elements: int64 tensor of shape (elements_capacity, 2) (default: its rows).  Without a d_elements of the caller's,
        one of ``elements_capacity`` records is made, and without that number either it is sized from a layout-only first
        call, whose 48-byte result is waited for.  elements=False: the layout-only form alone (d_elements None).
        d_elements_select: uint8[48] that receives the ``msj_select_documents_result`` of the element records, for
        ``string_column`` over them (default: a new one).  Returns (``MsjArrayColumnResult``, d_offsets, d_valid, d_elements,
        d_elements_select) -- blocking for the 48-byte result; with sync=False the device tensor that holds it, nothing
        waited for."""
        d_col = d_fields[p]
        _check_records(d_col, "the records of a path")
        n, numbers_capacity = int(n), int(numbers_capacity)
        capacity, d_offsets, d_valid = self._column_rows(d_col, d_offsets, d_valid, capacity)
        d_result, d_elements_select = self._result(d_result), self._result(d_elements_select)

        def call(room, d_out):
            rc = self.lib.msj_array_column_device(
                self.ctx, _ptr(d_idx), n, _ptr(d_type), _ptr(d_depth), _ptr(d_match), _ptr(d_end), _ptr(d_flags), _ptr(d_doc_first),
                _ptr(d_docs), _opt(d_numbers if numbers_capacity else None), numbers_capacity, _opt(d_numbers_result), _ptr(d_col),
                _ptr(d_select_result), _ptr(d_offsets), _ptr(d_valid), capacity, _opt(d_out), room, _ptr(d_result), _ptr(d_elements_select),
                self._stream())
            if rc != 0:
                raise RuntimeError(f"msj_array_column_device failed: {rc}")

        res, (d_elements,) = self._sized_call(call, _lib.MsjArrayColumnResult, d_result, "n_elements", elements, (d_elements,),
                                              elements_capacity, 2, sync)
        return res, d_offsets, d_valid, d_elements, d_elements_select

    def select_elements(self, paths, d_buf, length, d_idx, n, d_type, d_depth, d_match, d_end, d_flags, d_rows, d_rows_select,
                        d_numbers=None, numbers_capacity=0, d_numbers_result=None, d_fields=None, capacity=None, d_result=None,
                        sync=True):
        """Fields by path inside the elements of a list column (``msj_select_elements_device``): one 16-byte ``msj_field``
        per (path, element), path-major, aligned with the list column's offsets.  paths: from ``compile_paths``; the window,
        the token arrays and the number records with their result: those ``array_column`` ran over; d_rows: its d_elements,
        int64 of shape (rows, 2); d_rows_select: its d_elements_select, read on the device.  d_fields: int64 tensor of shape
        (n_paths, capacity, 2) as for ``select_documents`` -- default one row per record of d_rows.  Returns
        (``MsjSelectDocumentsResult``, d_fields) -- blocking for the 48-byte result; with sync=False the device tensor that
        holds it, nothing waited for.  That tensor is what ``string_column`` takes as d_select_result for any of the columns."""
        _check_records(d_rows, "the element records")
        n, length, numbers_capacity = int(n), int(length), int(numbers_capacity)
        if d_fields is None:
            capacity = d_rows.shape[0] if capacity is None else int(capacity)
            d_fields = torch.empty((paths.n_paths, max(capacity, 1), 2), dtype=torch.int64, device=self.device)
        elif capacity is None:
            capacity = d_fields.shape[1]
        if d_result is None:
            d_result = torch.zeros(48, dtype=torch.uint8, device=self.device)
        rc = self.lib.msj_select_elements_device(
            self.ctx, paths.handle, _ptr(d_buf), length, _ptr(d_idx), n, _ptr(d_type), _ptr(d_depth), _ptr(d_match), _ptr(d_end), _ptr(d_flags),
            _opt(d_numbers if numbers_capacity else None), numbers_capacity,
            _opt(d_numbers_result), _ptr(d_rows), _ptr(d_rows_select), _ptr(d_fields),
            int(capacity), _ptr(d_result), self._stream())
        if rc != 0:
            raise RuntimeError(f"msj_select_elements_device failed: {rc}")
        if not sync:
            return d_result, d_fields
        return _lib.MsjSelectDocumentsResult.from_buffer_copy(d_result.cpu().numpy().tobytes()), d_fields

    def array_elements(self, d_idx, n, d_type, d_depth, d_match, d_end, d_flags, d_rows, d_rows_select, d_numbers=None, numbers_capacity=0,
                       d_numbers_result=None, d_offsets=None, d_valid=None, d_elements=None, capacity=None, elements_capacity=None,
                       elements=True, d_result=None, d_elements_select=None, sync=True):
        """The arrays inside list rows as a list column (``msj_array_elements_device``): ``array_column`` with element records
        as the rows -- a list of lists, or a list inside a list of structs.  The token arrays and the number records with
        their result: those the call that wrote the rows ran over; d_rows: ``array_column``'s (or this call's) d_elements, or
        one path of ``select_elements``' d_fields, int64 of shape (rows, 2); d_rows_select: the device
        ``msj_select_documents_result`` that goes with them, read on the device.  d_offsets: int64 tensor of capacity + 1
        entries, d_valid: uint8 tensor of capacity entries (default: new ones, capacity = the rows of d_rows); d_elements:
        int64 tensor of shape (elements_capacity, 2) (default: its rows).  Without a d_elements of the caller's, one of
        ``elements_capacity`` records is made, and without that number either it is sized from a layout-only first call,
        whose 48-byte result is waited for.  elements=False: the layout-only form alone (d_elements None).
        d_elements_select: uint8[48] that receives the ``msj_select_documents_result`` of the element records (default: a
        new one).  Returns (``MsjArrayColumnResult``, d_offsets, d_valid, d_elements, d_elements_select) -- blocking for the
        48-byte result; with sync=False the device tensor that holds it, nothing waited for."""
        _check_records(d_rows, "the records of the rows")
        n, numbers_capacity = int(n), int(numbers_capacity)
        capacity, d_offsets, d_valid = self._column_rows(d_rows, d_offsets, d_valid, capacity)
        d_result, d_elements_select = self._result(d_result), self._result(d_elements_select)

        def call(room, d_out):
            rc = self.lib.msj_array_elements_device(
                self.ctx, _ptr(d_idx), n, _ptr(d_type), _ptr(d_depth), _ptr(d_match), _ptr(d_end), _ptr(d_flags),
                _opt(d_numbers if numbers_capacity else None), numbers_capacity, _opt(d_numbers_result), _ptr(d_rows), _ptr(d_rows_select),
                _ptr(d_offsets), _ptr(d_valid), capacity, _opt(d_out), room, _ptr(d_result), _ptr(d_elements_select), self._stream())
            if rc != 0:
                raise RuntimeError(f"msj_array_elements_device failed: {rc}")

        res, (d_elements,) = self._sized_call(call, _lib.MsjArrayColumnResult, d_result, "n_elements", elements, (d_elements,),
                                              elements_capacity, 2, sync)
        return res, d_offsets, d_valid, d_elements, d_elements_select

    def object_entries(self, d_idx, n, d_type, d_depth, d_match, d_end, d_flags, d_rows, d_rows_select, d_numbers=None, numbers_capacity=0,
                       d_numbers_result=None, d_offsets=None, d_valid=None, d_keys=None, d_values=None, capacity=None, entries_capacity=None,
                       entries=True, d_result=None, d_keys_select=None, d_values_select=None, sync=True):
        """An object's members as a map column (``msj_object_entries_device``): ``array_elements`` with objects as the rows and
        two records per entry.  The token arrays and the number records with their result: those the call that wrote the rows
        ran over; d_rows: any ``msj_field`` records, int64 of shape (rows, 2) -- one path of ``select_documents``' d_fields (the
        rows are the documents), the d_elements of an array call, one path of ``select_elements``' d_fields, or this call's own
        d_values; d_rows_select: the device ``msj_select_documents_result`` that goes with them, read on the device.
        d_offsets: int64 tensor of capacity + 1 entries, d_valid: uint8 tensor of capacity entries (default: new ones,
        capacity = the rows of d_rows); d_keys, d_values: int64 tensors of shape (entries_capacity, 2), both or neither
        (default: their rows).  Without record tensors of the caller's, two of ``entries_capacity`` records are made, and
        without that number either they are sized from a layout-only first call, whose 48-byte result is waited for.
        entries=False: the layout-only form alone (d_keys and d_values None).  d_keys_select, d_values_select: uint8[48] each,
        the ``msj_select_documents_result`` of the key and of the value records (default: new ones).  Returns
        (``MsjObjectEntriesResult``, d_offsets, d_valid, d_keys, d_values, d_keys_select, d_values_select) -- blocking for the
        48-byte result; with sync=False the device tensor that holds it, nothing waited for."""
        _check_records(d_rows, "the records of the rows")
        if (d_keys is None) != (d_values is None):
            raise ValueError("d_keys and d_values come together")
        n, numbers_capacity = int(n), int(numbers_capacity)
        capacity, d_offsets, d_valid = self._column_rows(d_rows, d_offsets, d_valid, capacity)
        d_result, d_keys_select, d_values_select = self._result(d_result), self._result(d_keys_select), self._result(d_values_select)

        def call(room, d_k, d_v):
            rc = self.lib.msj_object_entries_device(
                self.ctx, _ptr(d_idx), n, _ptr(d_type), _ptr(d_depth), _ptr(d_match), _ptr(d_end), _ptr(d_flags),
                _opt(d_numbers if numbers_capacity else None), numbers_capacity, _opt(d_numbers_result), _ptr(d_rows), _ptr(d_rows_select),
                _ptr(d_offsets), _ptr(d_valid), capacity, _opt(d_k), _opt(d_v), room, _ptr(d_result), _ptr(d_keys_select),
                _ptr(d_values_select), self._stream())
            if rc != 0:
                raise RuntimeError(f"msj_object_entries_device failed: {rc}")

        res, (d_keys, d_values) = self._sized_call(call, _lib.MsjObjectEntriesResult, d_result, "n_entries", entries, (d_keys, d_values),
                                                   entries_capacity, 2, sync)
        return res, d_offsets, d_valid, d_keys, d_values, d_keys_select, d_values_select

    def parse_document(self, d_buf, length, max_depth=100, exact_strings=False):
        """The whole chain for one document in a device buffer: stage 1, ``stage2_prep`` with partners, ``number_values``,
        ``validate`` and ``tape`` enqueued on one stream.  Returns stage 1's code if that is not 0, else
        (``MsjValidateResult``, ``MsjTapeResult``, d_tape, d_string_buf); the tape is specified when both codes are 0 (wrap
        it with ``mojo_simdjson_amd.document.Document.from_device``).  The token count and the number count size the later
        launches: they are the values read in between.  The string buffer has the reference's bound, 5 * length // 3 + 64
        bytes; exact_strings=True sizes it from a layout-only first call instead."""
        length = int(length)
        d_idx = torch.empty(length + 3 + 4, dtype=torch.int32, device=self.device)
        d_carry = self.new_carry()
        self.index(d_buf, d_idx, d_carry, length=length)
        carry = self.fetch(d_carry)
        if carry.code != 0:
            return int(carry.code)
        n = int(carry.count)
        d_type, d_depth, _, d_match, d_end, d_flags = self.stage2_prep(d_buf, length, d_idx, n, match=True)
        # (a layout pass of the number call: how many records the document needs)
        _, num = self.number_values(d_buf, length, d_idx, n, d_flags, capacity=0)
        cap = int(num.n_numbers)
        d_numbers, d_num = self.number_values(d_buf, length, d_idx, n, d_flags, capacity=cap, sync=False)
        d_verdict = self.validate(d_buf, length, d_idx, n, d_type, d_depth, d_match, d_end, d_flags, d_num, max_depth, sync=False)
        args = (d_buf, length, d_idx, n, d_type, d_depth, d_match, d_end, d_flags, d_numbers, cap)
        string_capacity = None
        if exact_strings:
            layout, d_tape, _ = self.tape(*args, d_verdict=d_verdict, strings=False)
            string_capacity = int(layout.string_bytes)
            tres, d_tape, d_sbuf = self.tape(*args, d_verdict=d_verdict, d_tape=d_tape, string_capacity=string_capacity)
        else:
            tres, d_tape, d_sbuf = self.tape(*args, d_verdict=d_verdict)
        verdict = _lib.MsjValidateResult.from_buffer_copy(d_verdict.cpu().numpy().tobytes())
        return verdict, tres, d_tape, d_sbuf

    def set_wait_ticks(self, ticks):
        """Test hook: bound of the single-pass kernel's inter-workgroup waits in 10 ns ticks (default 2 s)."""
        self.lib.msj_debug_set_wait_ticks(self.ctx, int(ticks))

    def fallback_count(self):
        """How often this context re-issued a call through the two-pass kernels after an expired wait."""
        return int(self.lib.msj_fallback_count(self.ctx))

    def fetch(self, d_carry):
        """Blocking read-back of a device ``msj_carry``."""
        out = _lib.MsjCarry()
        rc = self.lib.msj_carry_fetch(self.ctx, _ptr(d_carry), ctypes.byref(out), self._stream())
        if rc != 0:
            raise RuntimeError(f"msj_carry_fetch failed: {rc}")
        return out

