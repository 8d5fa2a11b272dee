// Stand-alone program (its own main; built by tests/test_raw_column_sanitizers.py with -fsanitize=address,undefined): the
// host form of msj_raw_column_device's arithmetic (tests/raw_column_math_host.cpp over csrc/raw_column_math.h) on arrays and
// records from anywhere.  A small lexer makes honest arrays for a pinned window; then, round after round, the arrays are
// damaged -- a d_idx that does not ascend, d_end beyond len, flags and types from a generator -- and the records are
// hostile: tokens at and past n, containers whose partner lies at or in front of the token or at or past n, records with
// codes.  Every array is a std::vector of exactly its size, so a read or a write outside is the sanitizer's to report.
// Asserted here: the counts add up, the offsets ascend by the rows' lengths, total_bytes is their sum, nothing past the
// capacities is written.  NOT part of the product.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../raw_column_math_host.cpp"

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
    return rng_state;
}

struct Win {
    std::vector<uint8_t> buf, type, flags;
    std::vector<uint32_t> idx, end, match;
};

// honest arrays for valid JSON text: a structural per bracket, comma, colon and per first byte of a scalar
Win lex(const std::string &text) {
    Win w;
    w.buf.assign(text.begin(), text.end());
    std::vector<uint32_t> open;
    for (size_t p = 0; p < text.size();) {
        const char c = text[p];
        if (c == ' ' || c == '\n' || c == '\t' || c == '\r') {
            p++;
            continue;
        }
        const uint32_t i = (uint32_t)w.idx.size();
        w.idx.push_back((uint32_t)p), w.type.push_back((uint8_t)c), w.match.push_back(0xFFFFFFFFu);
        if (c == '"') {
            size_t q = p + 1;
            while (text[q] != '"') q += text[q] == '\\' ? 2 : 1;
            w.end.push_back((uint32_t)q), w.flags.push_back(1);
            p = q + 1;
        } else if (c == '-' || (c >= '0' && c <= '9')) {
            size_t q = p + 1;
            while (q < text.size() && std::string("0123456789.eE+-").find(text[q]) != std::string::npos) q++;
            const bool far = q - p > 1024;
            w.end.push_back(far ? 0u : (uint32_t)q), w.flags.push_back(far ? 4 | 128 : 4);
            p = q;
        } else {
            w.end.push_back(0), w.flags.push_back(0);
            if (c == '{' || c == '[') open.push_back(i);
            if (c == '}' || c == ']') w.match[i] = open.back(), w.match[open.back()] = i, open.pop_back();
            p += c == 't' || c == 'n' ? 4 : c == 'f' ? 5 : 1;
        }
    }
    return w;
}

int failures = 0;
#define CHECK(x)                                                     \
    do {                                                             \
        if (!(x)) printf("FAILED %s (line %d)\n", #x, __LINE__), failures++; \
    } while (0)

void run(const Win &w, uint64_t len, const std::vector<msj_field> &rows, uint32_t flags, uint64_t bytes_capacity, bool layout_only) {
    const uint64_t R = rows.size(), n = w.idx.size();
    msj_select_documents_result sel{};
    sel.n_documents = R;
    std::vector<uint64_t> offsets(R + 1, 0x7777777777777777ull);
    std::vector<uint8_t> valid(R ? R : 1, 0x77), bytes(bytes_capacity ? bytes_capacity : 1, 0x77);
    msj_raw_column_result out;
    rcm_raw_column(w.buf.data(), len, w.idx.data(), n, w.type.data(), w.end.data(), w.flags.data(), rows.data(), &sel, offsets.data(),
                   valid.data(), R, layout_only ? nullptr : bytes.data(), layout_only ? 0 : bytes_capacity, flags, &out);
    CHECK(out.code == 0 || out.code == MSJ_CAPACITY);
    CHECK(out.n_rows == R && out.flags == flags && offsets[0] == 0);
    uint64_t values = 0, coded = 0;
    for (uint64_t k = 0; k < R; k++) {
        CHECK(valid[k] <= 1 && offsets[k + 1] >= offsets[k]);
        if (!valid[k]) CHECK(offsets[k + 1] == offsets[k]);
        values += valid[k], coded += rows[k].code != 0;
    }
    CHECK(values == out.n_values && out.n_containers <= out.n_values && values + out.n_other + coded == R);
    CHECK(out.total_bytes == offsets[R]);
    CHECK((out.code == MSJ_CAPACITY) == (!layout_only && out.total_bytes > bytes_capacity));
}

std::vector<msj_field> hostile_rows(const Win &w, uint64_t count) {
    const uint64_t n = w.idx.size();
    std::vector<msj_field> rows;
    for (uint64_t k = 0; k < count; k++) {
        msj_field f{};
        const uint64_t pick = rnd() % 10;
        f.token = pick == 0 ? (uint32_t)n : pick == 1 ? (uint32_t)(n + rnd() % 1000) : pick == 2 ? 0xFFFFFFFFu : (uint32_t)(rnd() % (n + 1));
        const char kinds[] = {'{', '[', '"', 'l', 'd', 't', 'f', 'n', 0};
        f.type = (uint8_t)kinds[rnd() % 9];
        switch (rnd() % 6) {
            case 0: f.bits = f.token; break;                           // the partner is the token
            case 1: f.bits = f.token ? rnd() % f.token : 0; break;     // in front of it
            case 2: f.bits = n + rnd() % 3; break;                     // at or past n
            case 3: f.bits = rnd(); break;
            case 4: f.bits = f.token < n ? w.match[f.token] : 0; break;  // d_match as it is (garbage after damage)
            default: f.bits = f.token + 1 + rnd() % 8; break;
        }
        f.code = rnd() % 7 == 0 ? (uint16_t)(17 + rnd() % 4) : 0;
        rows.push_back(f);
    }
    return rows;
}

}  // namespace

int main() {
    std::string big(1025, '7');
    const std::string text = "{\"a\": [1, 2.5e3, {\"b\": \"x , ] }\\\"\\\\\"}, [], {}], \"n\": null, \"t\": true,\r\n\t\"f\": false, \"big\": " + big +
                             "   \n}\n[[[[[1]]]]] \"tail\" -0.5\n" + big;
    const Win honest = lex(text);
    const uint64_t n = honest.idx.size();
    // honest arrays, honest records for every value: in bounds and the root is the text of the first document
    {
        std::vector<msj_field> rows;
        for (uint32_t i = 0; i < n; i++) {
            msj_field f{};
            f.token = i, f.type = honest.type[i], f.bits = honest.match[i];
            if (f.type != '}' && f.type != ']') rows.push_back(f);
        }
        for (uint32_t flags = 0; flags < 2; flags++) run(honest, text.size(), rows, flags, text.size() * n, false);
    }
    for (int round = 0; round < 600; round++) {
        Win w = honest;
        uint64_t len = text.size();
        const int damage = round % 6;
        if (damage == 1)
            for (int j = 0; j < 8; j++) std::swap(w.idx[rnd() % n], w.idx[rnd() % n]);  // a d_idx that does not ascend
        if (damage == 2)
            for (auto &e : w.end) e = rnd() % 3 ? e : (uint32_t)(len + rnd() % 5000);  // d_end beyond len
        if (damage == 3)
            for (uint64_t i = 0; i < n; i++) w.flags[i] = (uint8_t)rnd(), w.type[i] = (uint8_t)"tfn{}[]\",:0-x"[rnd() % 13];
        if (damage == 4) {
            for (auto &m : w.match) m = (uint32_t)rnd();  // d_match garbage
            for (auto &x : w.idx) x = rnd() % 4 ? x : (uint32_t)rnd();
        }
        if (damage == 5) len = rnd() % (text.size() + 1), w.buf.resize(len ? len : 1);  // a window shorter than its index says
        const std::vector<msj_field> rows = hostile_rows(w, 1 + rnd() % 300);
        for (uint32_t flags = 0; flags < 2; flags++) {
            run(w, len, rows, flags, 0, true);
            run(w, len, rows, flags, rnd() % 4096, false);
            run(w, len, rows, flags, 1 << 20, false);
        }
    }
    if (failures) return 1;
    printf("raw_column_sanitize ok\n");
    return 0;
}
