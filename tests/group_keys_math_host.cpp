// Test-only harness: compiles mojo_simdjson_amd/csrc/group_keys_math.h for the host (g++), so that the arithmetic of
// msj_bucket_rows_device and msj_group_keys_device -- the same floor, part encoders, decode and codes the kernels run
// (csrc/group_keys_kernel.hip) -- is checked on a CPU-only box against the definition written in Python with Fraction
// (tests/test_group_keys_math.py), and so that the GPU tests have an expected value.  The keys call goes block by block as
// the kernel does: 256 rows built in a tile, the tile copied out in 16-byte pieces and a tail byte by byte.  NOT part of the
// product.
#include <string.h>

#include <vector>

#include "../include/msj_stage1.h"
#include "../mojo_simdjson_amd/csrc/group_keys_math.h"

using namespace msj::gkeys;

namespace {
bool aligned_to(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
constexpr uint32_t kTwinRows = 256;
}  // namespace

extern "C" {

// the pieces on their own
int32_t gkm_floor_of_double(uint64_t bits, int64_t *f, int32_t *whole) {
    bool w;
    const bool ok = floor_of_double(bits, f, &w);
    *whole = w;
    return ok;
}
int32_t gkm_bucket_floor(int64_t f, int64_t width, int64_t origin, int64_t *s) { return bucket_floor(f, (uint64_t)width, origin, s); }
uint32_t gkm_bucket_record(const msj_field *in, int64_t width, int64_t origin, msj_field *out) { return bucket_record(*in, width, origin, *out); }
int32_t gkm_encode_number(const msj_field *f, uint8_t *out) { return encode_number(*f, out); }
int32_t gkm_encode_code(int32_t code, uint8_t *out) { return encode_code(code, out); }
int32_t gkm_decode_number(const uint8_t *p, uint32_t *type, uint64_t *bits) { return decode_number(p, type, bits); }
int32_t gkm_decode_code(const uint8_t *p, int32_t *code) { return decode_code(p, code); }
uint32_t gkm_part_width(uint32_t kind) { return part_width(kind); }

// msj_bucket_rows_device, serially.  The select result: a host copy of the device words.  -> 0, or what the entry point refuses
// on the host, in the header's order, with nothing written
int32_t gkm_bucket_rows(const msj_field *rows, const msj_select_documents_result *sel, int64_t width, int64_t origin, uint32_t flags, msj_field *out,
                        uint64_t capacity, msj_bucket_rows_result *res, msj_select_documents_result *out_sel) {
    if (!res || !sel) return MSJ_ERR_BAD_ARGUMENT;
    if (capacity > 0 && (!rows || !out)) return MSJ_ERR_BAD_ARGUMENT;
    if (bad_bucket(width, flags)) return MSJ_ERR_BAD_ARGUMENT;
    if (capacity >= (1ull << 40)) return MSJ_CAPACITY;
    if (out && rows && out != rows) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(rows), b = reinterpret_cast<uintptr_t>(out);
        if (a < b + 16 * capacity && b < a + 16 * capacity) return MSJ_ERR_BAD_ARGUMENT;
    }
    if ((const void *)res == (const void *)sel || (const void *)res == (const void *)out_sel || out_sel == sel) return MSJ_ERR_BAD_ARGUMENT;
    if (!aligned_to(rows, 16) || !aligned_to(out, 16) || !aligned_to(sel, 8) || !aligned_to(res, 8) || !aligned_to(out_sel, 8))
        return MSJ_ERR_BAD_ARGUMENT;

    const uint64_t R = sel->n_documents;
    const bool skip = sel->code != 0, over = !skip && msj::scol::rows_over(R, capacity);
    msj_bucket_rows_result r;
    memset(&r, 0, sizeof r);
    r.code = skip ? sel->code : over ? MSJ_CAPACITY : 0;
    r.n_rows = skip ? 0 : R;
    uint64_t n_no_bits = 0;
    if (!skip && !over)
        for (uint64_t k = 0; k < R; k++) {
            msj_field o;
            const uint32_t outcome = bucket_record(rows[k], width, origin, o);
            out[k] = o;
            r.n_bucketed += outcome == kBucketed, r.n_range += outcome == kRange, r.n_skipped += outcome == kNoBits, r.n_other += outcome == kOther;
            n_no_bits += (o.flags & kFieldNoBits) != 0;
        }
    *res = r;
    if (out_sel) {
        memset(out_sel, 0, sizeof *out_sel);
        out_sel->code = r.code, out_sel->n_documents = skip || over ? 0 : R, out_sel->n_paths = 1, out_sel->n_found = r.n_bucketed;
        out_sel->n_no_bits = n_no_bits;
    }
    return 0;
}

// msj_group_keys_device, block by block
int32_t gkm_group_keys(const msj_key_part *parts, uint32_t n_parts, uint64_t stride, const msj_select_documents_result *sel, uint64_t *offsets,
                       uint8_t *valid, uint8_t *bytes, uint64_t capacity, uint64_t bytes_capacity, msj_group_keys_result *res) {
    if (!res || !sel || !parts) return MSJ_ERR_BAD_ARGUMENT;
    if (n_parts == 0 || n_parts > kMaxParts) return MSJ_ERR_BAD_ARGUMENT;
    for (uint32_t j = 0; j < n_parts; j++)
        if (bad_part(parts[j].kind, parts[j].flags)) return MSJ_ERR_BAD_ARGUMENT;
    for (uint32_t j = 0; j < n_parts; j++)
        if (stride > 0 && !parts[j].d_column) return MSJ_ERR_BAD_ARGUMENT;
    if (capacity > 0 && (!offsets || !valid || !bytes)) return MSJ_ERR_BAD_ARGUMENT;
    if ((const void *)res == (const void *)sel) return MSJ_ERR_BAD_ARGUMENT;
    for (uint32_t j = 0; j < n_parts; j++)
        if (!aligned_to(parts[j].d_column, parts[j].kind == kNumber ? 16 : 4)) return MSJ_ERR_BAD_ARGUMENT;
    if (!aligned_to(bytes, 16) || !aligned_to(offsets, 8) || !aligned_to(sel, 8) || !aligned_to(res, 8)) return MSJ_ERR_BAD_ARGUMENT;

    uint32_t W = 0;
    for (uint32_t j = 0; j < n_parts; j++) W += part_width(parts[j].kind);
    const uint64_t R = sel->n_documents;
    msj_group_keys_result r;
    memset(&r, 0, sizeof r);
    r.code = head_code(sel->code, R, stride, capacity, W, bytes_capacity, MSJ_CAPACITY);
    r.n_rows = sel->code != 0 ? 0 : R;
    r.key_width = W;
    if (r.code == 0) {
        std::vector<uint8_t> tile(kTwinRows * kMaxWidth);
        for (uint64_t v = 0; v * kTwinRows < R; v++) {
            const uint32_t rows_here = R - v * kTwinRows < kTwinRows ? (uint32_t)(R - v * kTwinRows) : kTwinRows;
            for (uint32_t t = 0; t < rows_here; t++) {
                const uint64_t k = v * kTwinRows + t;
                uint8_t *p = tile.data() + t * W;
                bool any_null = false, ok = true;
                for (uint32_t j = 0; j < n_parts; j++) {
                    bool null;
                    if (parts[j].kind == kNumber) null = encode_number(static_cast<const msj_field *>(parts[j].d_column)[k], p), p += kNumberBytes;
                    else null = encode_code(static_cast<const int32_t *>(parts[j].d_column)[k], p), p += kCodeBytes;
                    any_null |= null;
                    ok &= !null || (parts[j].flags & kNullIsGroup) != 0;
                }
                offsets[k] = k * W, valid[k] = ok ? 1 : 0;
                r.n_keys += ok, r.n_null_rows += any_null;
            }
            const uint64_t first = v * kTwinRows * W;
            const uint32_t count = rows_here * W;
            uint32_t at = 0;
            for (; at + 16 <= count; at += 16) memcpy(bytes + first + at, tile.data() + at, 16);
            for (; at < count; at++) bytes[first + at] = tile[at];
        }
        r.bytes_len = R * W;
        if (offsets) offsets[R] = R * W;
    }
    *res = r;
    return 0;
}

}  // extern "C"
