// Stand-alone program (its own main; built by tests/test_filter_rows_sanitizers.py with -fsanitize=address,undefined): the
// host form of the arithmetic of msj_predicates_create, msj_filter_rows_device and msj_take_rows_device
// (tests/filter_rows_math_host.cpp over csrc/filter_rows_math.h) on arrays from anywhere.  The pinned numbers and strings of
// tests/test_filter_rows_math.py -- integers and doubles around 2^53 and 2^63, escapes, a surrogate pair, a span that ends at
// the window's end and one a byte past it, damaged escapes -- and then, round after round, records with bits, types, flags and
// codes from a generator, list offsets that descend or exceed R, take indices at R - 1, R and 0xFFFFFFFF and repeated, a row
// count below and above the capacities, each capacity one short, the mask-only form.  Every array is a std::vector of exactly
// its size, so a read or a write outside is the sanitizer's to report.  Asserted here: the counts add up, the kept rows
// ascend and are the rows whose keep byte is set, the re-based offsets are the ranks, nothing past the capacities is
// written, a taken record is its source or the record of a missing value.  NOT part of the product.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../filter_rows_math_host.cpp"

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
    return rng_state;
}

int failures = 0;
#define CHECK(x)                                                     \
    do {                                                             \
        if (!(x)) printf("FAILED %s (line %d)\n", #x, __LINE__), failures++; \
    } while (0)

constexpr uint8_t kFill = 0x77;

uint64_t bits_of(double d) {
    uint64_t b;
    memcpy(&b, &d, 8);
    return b;
}
msj_field field(uint64_t bits, uint8_t type, uint8_t flags = 0, uint16_t code = 0, uint32_t token = 0) {
    msj_field f;
    f.bits = bits, f.token = token, f.type = type, f.flags = flags, f.code = code;
    return f;
}

struct Window {
    std::vector<uint8_t> data;
    std::vector<msj_field> strings;  // a record per body
};
Window pinned_window() {
    Window w;
    const std::string bodies[] = {"A", "\\u0041", "", "ab", "\\ud83d\\ude00x", "\\u20acz", "\\u0041\\u0041", "a\\u0000b", "q\\n\\t\\\"\\\\",
                                  "\\ude00", "ab\\u00zzcd", "abc\\u00", "ab\\", std::string(255, 'q'), std::string(256, 'q')};
    for (const std::string &b : bodies) {
        w.data.push_back('"');
        const bool escaped = b.find('\\') != std::string::npos;
        w.strings.push_back(field(w.data.size() | ((uint64_t)b.size() << 32), '"', escaped ? 2 : 0));
        w.data.insert(w.data.end(), b.begin(), b.end());
        w.data.push_back('"');
    }
    const std::string tail = "tail";
    w.data.push_back('"');
    w.strings.push_back(field(w.data.size() | ((uint64_t)tail.size() << 32), '"'));
    w.strings.push_back(field(w.data.size() | ((uint64_t)(tail.size() + 1) << 32), '"'));
    w.strings.push_back(field(w.data.size() | ((uint64_t)(tail.size() + 1) << 32), '"', 2));
    w.strings.push_back(field(0xFFFFFFFFFFFFFFFFull, '"', 2));
    w.data.insert(w.data.end(), tail.begin(), tail.end());
    w.data.shrink_to_fit();
    return w;
}

std::vector<msj_field> pinned_numbers() {
    std::vector<msj_field> v;
    const int64_t ints[] = {0, 1, -1, (1ll << 53) - 1, -((1ll << 53) - 1), 1ll << 53, -(1ll << 53), (1ll << 53) + 1, -((1ll << 53) + 1), INT64_MAX, INT64_MIN};
    const double doubles[] = {0.0, -0.0, 0.5, -0.5, 1.5, -1.5, 9007199254740992.0, -9007199254740992.0, 9007199254740994.0, -9007199254740994.0,
                              9.223372036854775807e18, -9.223372036854775807e18, 5e-324, 1.7976931348623157e308, -1.7976931348623157e308};
    for (int64_t i : ints) v.push_back(field((uint64_t)i, 'l'));
    for (double d : doubles) v.push_back(field(bits_of(d), 'd'));
    v.push_back(field(0x7FF8000000000000ull, 'd'));  // a NaN, +inf, -inf: no number call writes them
    v.push_back(field(0x7FF0000000000000ull, 'd'));
    v.push_back(field(0xFFF0000000000000ull, 'd'));
    v.push_back(field(0, 'l', 64));
    v.push_back(field(0, 'd', 64));
    for (uint8_t t : {'{', '[', 't', 'f', 'n', 'x'}) v.push_back(field(3, t));
    for (uint16_t c : {20, 17, 3}) v.push_back(field(0, 0, 0, c, 0xFFFFFFFFu));
    return v;
}

std::vector<std::string> operands() {
    return {"", "A", "ab", "abc", std::string(255, 'q'), "\xf0\x9f\x98\x80", "\xf0\x9f", "\xe2", "\xe2\x82", "\xe2\x82\xac", "AA", std::string("a\0b", 3),
            std::string("a\0", 2), "tail", "tai", "ab\\"};
}

// predicates from a generator over the pinned operands: always valid
std::vector<uint8_t> draw_predicates(uint32_t n_columns, const std::vector<std::string> &ops, std::vector<msj_predicate> &specs) {
    const uint32_t n = 1 + (uint32_t)(rnd() % 16);
    specs.assign(n, msj_predicate{});
    const std::vector<msj_field> numbers = pinned_numbers();
    for (msj_predicate &s : specs) {
        s.column = (uint32_t)(rnd() % n_columns);
        s.op = (uint32_t)(rnd() % 9);
        s.flags = (uint32_t)(rnd() % 2);
        if (s.op == kType) s.operand_bits = 1 + rnd() % 255;
        if (s.op >= kNumEq && s.op <= kNumGe) {
            const msj_field &f = numbers[rnd() % 26];  // (the finite ones)
            s.operand_bits = f.bits;
            if (f.type == 'd') s.flags |= kOperandDouble;
        }
        if (s.op >= kStrEq) {
            const std::string &o = ops[rnd() % ops.size()];
            s.operand_len = (uint32_t)o.size(), s.operand_bytes = reinterpret_cast<const uint8_t *>(o.data());
        }
    }
    std::vector<uint8_t> blob(frm_predicates_bytes());
    CHECK(frm_compile(specs.data(), n, (uint32_t)(rnd() % 2), blob.data()) == 0);
    return blob;
}

// One filter call and one take call over `fields` (n_columns * stride records), every output at its exact size
void run(const Window &w, const std::vector<msj_field> &fields, uint64_t stride, uint32_t n_columns, uint64_t R, uint64_t capacity, bool mask_only,
         const std::vector<uint64_t> *offsets, const uint64_t *list_n_rows, int32_t sel_code, const std::vector<uint8_t> &blob,
         std::vector<uint32_t> take, int take_form) {
    msj_select_documents_result sel{};
    sel.code = sel_code, sel.n_documents = R, sel.n_paths = n_columns;
    std::vector<uint8_t> keep(capacity, kFill);
    std::vector<uint32_t> kept(mask_only ? 0 : capacity, 0x77777777u);
    const uint64_t list_rows = offsets ? offsets->size() - 1 : 0;
    std::vector<uint64_t> list_out(offsets ? list_rows + 1 : 0, 0x7777777777777777ull);
    msj_filter_rows_result res;
    msj_select_documents_result ksel;
    const int rc = frm_filter_rows(blob.data(), w.data.data(), w.data.size(), fields.data(), stride, n_columns, &sel, keep.data(),
                                   mask_only ? nullptr : kept.data(), capacity, offsets ? offsets->data() : nullptr, list_rows, list_n_rows,
                                   offsets ? list_out.data() : nullptr, &res, &ksel);
    CHECK(rc == 0);
    const bool over = R > capacity || R >= (1ull << 31);
    if (sel_code != 0 || over) {
        CHECK(res.code == (sel_code ? sel_code : MSJ_CAPACITY) && res.n_kept == 0 && ksel.code == res.code && ksel.n_documents == 0);
        for (uint8_t x : keep) CHECK(x == kFill);
        for (uint32_t x : kept) CHECK(x == 0x77777777u);
        for (uint64_t x : list_out) CHECK(x == 0x7777777777777777ull);
    } else {
        uint64_t n = 0;
        std::vector<uint64_t> rank(R + 1);
        for (uint64_t k = 0; k < R; k++) {
            CHECK(keep[k] <= 1);
            rank[k] = n;
            if (keep[k] && !mask_only) CHECK(kept[n] == k);
            n += keep[k];
        }
        rank[R] = n;
        CHECK(res.n_kept == n && res.n_rows == R && res.n_missing <= R && res.n_no_bits <= R && ksel.n_documents == n && ksel.n_found == n);
        for (uint64_t k = R; k < capacity; k++) CHECK(keep[k] == kFill);
        for (uint64_t k = n; k < kept.size(); k++) CHECK(kept[k] == 0x77777777u);
        const uint64_t P = list_n_rows ? *list_n_rows : list_rows;
        if (offsets && P <= list_rows) {
            CHECK(res.code == 0);
            for (uint64_t r = 0; r <= P; r++) CHECK(list_out[r] == rank[(*offsets)[r] < R ? (*offsets)[r] : R]);
            for (uint64_t r = P + 1; r <= list_rows; r++) CHECK(list_out[r] == 0x7777777777777777ull);
        } else if (offsets) {
            CHECK(res.code == MSJ_CAPACITY);
            for (uint64_t x : list_out) CHECK(x == 0x7777777777777777ull);
        }
        if (!mask_only && take_form == 0) take.assign(kept.begin(), kept.begin() + n);
    }
    // the take: out_capacity exact, one short, or K on the device one above the vector
    uint64_t K = take.size(), out_capacity = K;
    if (take_form == 2 && out_capacity) out_capacity--;
    if (take_form == 3) K++;
    const uint64_t Rt = take_form == 4 ? R : (R < stride ? R : stride);
    const uint64_t out_stride = out_capacity + rnd() % 3;
    msj_select_documents_result tsel{}, rsel{}, osel;
    tsel.n_documents = K, rsel.n_documents = Rt, rsel.code = sel_code;
    std::vector<msj_field> out((n_columns - 1) * out_stride + out_capacity, field(0x7777777777777777ull, 0x77, 0x77, 0x7777, 0x77777777u));
    msj_take_rows_result tres;
    frm_take_rows(take.data(), &tsel, fields.data(), stride, n_columns, &rsel, out.data(), out_stride, out_capacity, &tres, &osel);
    if (sel_code != 0 || K > out_capacity || Rt > stride) {
        CHECK(tres.code == (sel_code ? sel_code : MSJ_CAPACITY) && osel.code == tres.code && osel.n_documents == 0);
        for (const msj_field &f : out) CHECK(f.token == 0x77777777u);
        return;
    }
    CHECK(tres.code == 0 && tres.n_rows == K && osel.n_documents == K && osel.n_paths == n_columns && osel.n_found == tres.n_found);
    uint64_t found = 0, oor = 0;
    for (uint64_t j = 0; j < K; j++) {
        oor += take[j] >= Rt;
        for (uint32_t c = 0; c < n_columns; c++) {
            const msj_field &f = out[c * out_stride + j];
            if (take[j] >= Rt) CHECK(f.code == 20 && f.token == 0xFFFFFFFFu && f.bits == 0 && f.type == 0 && f.flags == 0);
            else CHECK(memcmp(&f, &fields[c * stride + take[j]], 16) == 0);
            found += f.code == 0;
        }
    }
    CHECK(found == tres.n_found && oor == tres.n_out_of_range);
}

}  // namespace

int main() {
    const Window w = pinned_window();
    const std::vector<std::string> ops = operands();
    std::vector<msj_field> pool = pinned_numbers();
    pool.insert(pool.end(), w.strings.begin(), w.strings.end());
    // every pinned record under every pinned operand and number, all ops, plain and negated
    for (const msj_field &operand : pinned_numbers()) {
        if ((operand.type != 'l' && operand.type != 'd') || operand.flags || !is_finite_bits(operand.bits)) continue;
        std::vector<msj_predicate> specs;
        for (uint32_t op = kNumEq; op <= kNumGe; op++)
            for (uint32_t neg = 0; neg < 2; neg++) specs.push_back(msj_predicate{0, op, neg | (operand.type == 'd' ? kOperandDouble : 0u), 0, operand.bits, nullptr});
        std::vector<uint8_t> blob(frm_predicates_bytes());
        CHECK(frm_compile(specs.data(), (uint32_t)specs.size(), 0, blob.data()) == 0);
        for (const msj_field &f : pool)
            for (uint32_t i = 0; i < specs.size(); i += 2) {
                const uint32_t a = frm_eval(blob.data(), i, &f, w.data.data(), w.data.size()), b = frm_eval(blob.data(), i + 1, &f, w.data.data(), w.data.size());
                CHECK(((a ^ b) & kHolds) == kHolds && (a & ~kHolds) == (b & ~kHolds));
            }
    }
    for (const std::string &o : ops) {
        std::vector<msj_predicate> specs;
        for (uint32_t op = kStrEq; op <= kStrPrefix; op++)
            specs.push_back(msj_predicate{0, op, 0, (uint32_t)o.size(), 0, reinterpret_cast<const uint8_t *>(o.data())});
        std::vector<uint8_t> blob(frm_predicates_bytes());
        CHECK(frm_compile(specs.data(), 2, 0, blob.data()) == 0);
        for (const msj_field &f : pool) {
            const uint32_t eq = frm_eval(blob.data(), 0, &f, w.data.data(), w.data.size()), pre = frm_eval(blob.data(), 1, &f, w.data.data(), w.data.size());
            CHECK(!(eq & kHolds) || (pre & kHolds));  // an equal value starts with the operand
        }
    }
    // 300 damaged inputs
    for (int round = 0; round < 300; round++) {
        const uint32_t n_columns = 1 + (uint32_t)(rnd() % 3);
        const uint64_t stride = rnd() % 40;
        std::vector<msj_field> fields(n_columns * stride);
        for (msj_field &f : fields) {
            f = pool[rnd() % pool.size()];
            if (rnd() % 4 == 0) f.bits = rnd();
            if (rnd() % 8 == 0) f.type = (uint8_t)rnd();
            if (rnd() % 8 == 0) f.flags = (uint8_t)rnd();
            if (rnd() % 16 == 0) f.code = (uint16_t)rnd();
        }
        fields.shrink_to_fit();
        std::vector<msj_predicate> specs;
        const std::vector<uint8_t> blob = draw_predicates(n_columns, ops, specs);
        const int form = round % 6;
        uint64_t capacity = form == 1 && stride ? stride - 1 : stride, R = stride;
        if (form == 2) R = rnd() % (stride + 1);
        if (form == 3) R = stride + 1 + rnd() % 3;
        std::vector<uint64_t> offsets(1 + rnd() % 12);
        for (uint64_t &o : offsets) o = rnd() % (R + 1);
        for (int hits = (int)(rnd() % 4); hits > 0; hits--) offsets[rnd() % offsets.size()] = rnd() % 2 ? R + 1 + rnd() % 4 : rnd();
        offsets.shrink_to_fit();
        const uint64_t list_rows = offsets.size() - 1, p_choices[] = {0, list_rows ? list_rows - 1 : 0, list_rows, list_rows + 1};
        const uint64_t P = p_choices[rnd() % 4];
        std::vector<uint32_t> take(rnd() % 50);
        for (uint32_t &t : take) t = (uint32_t)(rnd() % (R + 1));
        for (int hits = (int)(rnd() % 4); hits > 0 && !take.empty(); hits--) {
            const uint32_t choices[] = {(uint32_t)(R ? R - 1 : 0), (uint32_t)R, 0xFFFFFFFFu, take[0]};
            take[rnd() % take.size()] = choices[rnd() % 4];
        }
        take.shrink_to_fit();
        run(w, fields, stride, n_columns, R, capacity, form == 4, round % 3 ? &offsets : nullptr, round % 5 == 0 ? &P : nullptr, round % 41 == 0 ? 5 : 0,
            blob, take, (round / 6) % 5);
    }
    if (failures) return 1;
    printf("filter_rows_sanitize ok\n");
    return 0;
}
