// Test-only harness: compiles mojo_simdjson_amd/csrc/aggregate_math.h for the host (g++), so that the arithmetic of
// msj_aggregate_device -- the same value test, exponents, limbs, 128-bit recombination, final rounding and min / max rule the
// kernels run (csrc/aggregate_kernel.hip) -- is checked on a CPU-only box against the definition written in Python with
// Fraction and int (tests/test_aggregate_math.py), and so that the GPU tests have an expected value.  NOT part of the product.
#include <string.h>

#include <vector>

#include "../include/msj_stage1.h"
#include "../mojo_simdjson_amd/csrc/aggregate_math.h"

using namespace msj::agg;

extern "C" {

// the pieces on their own
uint32_t agm_value_kind(const msj_field *f) { return value_kind(*f); }
uint32_t agm_exp_key(uint32_t type, uint64_t bits) { return exp_key(type, bits); }
void agm_value_limbs(uint32_t type, uint64_t bits, uint32_t ekey, int64_t *l) { value_limbs(type, bits, ekey, l); }
void agm_int_limbs(int64_t v, int64_t *l) { int_limbs(v, l); }
void agm_recombine(int64_t a0, int64_t a1, int64_t a2, uint64_t *lo, int64_t *hi) {
    const S128 s = recombine(a0, a1, a2);
    *lo = s.lo, *hi = s.hi;
}
uint64_t agm_round_scaled(uint64_t lo, int64_t hi, int32_t scale, uint32_t *infinite) {
    bool inf;
    const uint64_t bits = round_scaled(S128{lo, hi}, scale, &inf);
    *infinite = inf;
    return bits;
}
int32_t agm_replaces(int32_t want, uint32_t t_new, uint64_t b_new, uint32_t t_old, uint64_t b_old) { return replaces(want, t_new, b_new, t_old, b_old); }

// The whole call, serially.  sel: a host copy of the device words; codes may be NULL.  split_minmax = 0: the minimum and
// the maximum by the merge rule, row after row (the definition); 1: as the kernels find them, ints and doubles apart and
// merged at the end.  -> 0, or -1 for what the entry point refuses on the host (the column count)
int agm_aggregate(const msj_field *fields, uint64_t stride, uint32_t n_columns, const msj_select_documents_result *sel, const int32_t *codes,
                  uint64_t G, msj_aggregate *groups, uint64_t groups_capacity, msj_aggregate_result *res, int split_minmax) {
    if (n_columns == 0 || n_columns > kMaxColumns) return -1;
    memset(res, 0, sizeof *res);
    if (sel->code != 0) {
        res->code = sel->code;
        return 0;
    }
    const uint64_t R = sel->n_documents;
    res->n_rows = R, res->n_groups = G;
    if (rows_over(R, stride) || groups_over(G, groups_capacity)) {
        res->code = MSJ_CAPACITY;
        return 0;
    }
    for (uint64_t k = 0; k < R; k++) res->n_ungrouped += group_of(codes, k, G) < 0;
    struct Best {
        uint32_t type;
        uint64_t bits;
    };
    for (uint32_t c = 0; c < n_columns; c++) {
        const msj_field *col = fields + (uint64_t)c * stride;
        std::vector<Acc> acc(G, Acc{});
        std::vector<Best> lo(G, Best{0, 0}), hi(G, Best{0, 0});
        for (uint64_t k = 0; k < R; k++) {
            const int64_t g = group_of(codes, k, G);
            if (g < 0) continue;
            const msj_field f = col[k];
            const uint32_t kind = value_kind(f);
            acc[g].n_rows++;
            res->n_skipped += kind == kSkipped;
            if (kind != kValue) continue;
            const bool first = acc[g].n_values == 0;
            acc_note(acc[g], f.type, f.bits);
            if (first || replaces(-1, f.type, f.bits, lo[g].type, lo[g].bits)) lo[g] = Best{f.type, f.bits};
            if (first || replaces(1, f.type, f.bits, hi[g].type, hi[g].bits)) hi[g] = Best{f.type, f.bits};
        }
        for (uint64_t k = 0; k < R; k++) {
            const int64_t g = group_of(codes, k, G);
            if (g < 0) continue;
            const msj_field f = col[k];
            if (value_kind(f) != kValue) continue;
            int64_t l[3];
            pass2_limbs(acc[g].n_double, acc[g].ekey, f.type, f.bits, l);
            for (int i = 0; i < 3; i++) acc[g].a[i] = (int64_t)((uint64_t)acc[g].a[i] + (uint64_t)l[i]);
        }
        for (uint64_t g = 0; g < G; g++) {
            msj_aggregate r = finish_group<msj_aggregate>(acc[g]);
            if (!split_minmax && r.n_values) r.min_type = (uint8_t)lo[g].type, r.min_bits = lo[g].bits, r.max_type = (uint8_t)hi[g].type, r.max_bits = hi[g].bits;
            groups[(uint64_t)c * groups_capacity + g] = r;
            res->n_values += r.n_values, res->flags |= r.flags;
        }
    }
    return 0;
}

}  // extern "C"
