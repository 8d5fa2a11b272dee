// Test-only program (its own main): the host twin of msj_array_column_device (tests/array_column_math_host.cpp, and through
// it mojo_simdjson_amd/csrc/array_column_math.h) under AddressSanitizer + UndefinedBehaviorSanitizer, fed by the select twin
// (tests/select_math_host.cpp).  tests/test_array_column_sanitizers.py builds it with -fsanitize=address,undefined and runs
// it.  Every array is allocated at its exact size, so a read or a store one element out shows.  A small serial tokenizer
// below stands in for stage 1 + prep + split: it only has to give arrays of the right shape, also for the mutated inputs and
// the hostile records, where the call must stay in bounds whatever they hold.
#include <stdio.h>
#include <stdlib.h>

#include <memory>
#include <string>
#include <vector>

#include "../array_column_math_host.cpp"
#include "../select_math_host.cpp"

namespace {

struct Tokens {
    std::vector<uint32_t> idx, mat, end, first;
    std::vector<uint8_t> typ, flags;
    std::vector<int32_t> dep;
};

Tokens tokenize(const std::string &s) {
    Tokens t;
    std::vector<uint32_t> open;
    int32_t depth = 0;
    for (size_t p = 0; p < s.size(); p++) {
        const uint8_t c = (uint8_t)s[p];
        if (c == ' ' || c == '\n') continue;
        const uint32_t i = (uint32_t)t.idx.size(), start = (uint32_t)p;
        uint32_t e = 0, m = kNoPartner;
        uint8_t fl = 0;
        int32_t d = depth;
        if (c == '{' || c == '[') {
            open.push_back(i);
            depth++;
        } else if (c == '}' || c == ']') {
            d = --depth;
            if (!open.empty()) {
                m = open.back();
                open.pop_back();
                t.mat[m] = i;
            }
        } else if (c == '"') {
            fl = 1;
            size_t q = p + 1;
            while (q < s.size() && s[q] != '"') {
                if (s[q] == '\\') fl |= 2, q++;
                q++;
            }
            e = (uint32_t)(q < s.size() ? q : s.size());
            p = e;
        } else if (c != ':' && c != ',') {
            size_t q = p;
            while (q < s.size() && !strchr(",:{}[] \n\"", s[q])) q++;
            if (c == '-' || (c >= '0' && c <= '9')) fl = 4 | (s.substr(p, q - p).find_first_of(".eE") != std::string::npos ? 8 : 0);
            e = (uint32_t)q;
            p = q - 1;
        }
        if (d == 0 && c != '}' && c != ']') t.first.push_back(i);
        t.idx.push_back(start);
        t.typ.push_back(c), t.dep.push_back(d), t.mat.push_back(m), t.end.push_back(e), t.flags.push_back(fl);
    }
    return t;
}

int fail(const char *what) {
    printf("array_column_sanitize: %s\n", what);
    return 1;
}

struct Out {
    std::vector<uint64_t> offsets;
    std::vector<uint8_t> valid;
    std::unique_ptr<msj_field[]> elements;  // (new[] of 0 records is no NULL: a NULL d_elements is the layout-only form)
    msj_array_column_result res;
    msj_select_documents_result esel;
};

// one call with every array at its exact size; layout_only: d_elements NULL
Out run(const Tokens &t, const msj_documents_result &docs, const std::vector<msj_number> &numbers, const msj_numbers_result *nr,
        const std::vector<msj_field> &column, const msj_select_documents_result &sel, uint64_t capacity, uint64_t room, bool layout_only) {
    Out o;
    o.offsets.resize(capacity + 1), o.valid.resize(capacity);
    if (!layout_only) o.elements.reset(new msj_field[room]);
    acm_array_column(t.idx.data(), t.idx.size(), t.typ.data(), t.dep.data(), t.mat.data(), t.end.data(), t.flags.data(), t.first.data(), &docs,
                     numbers.empty() ? nullptr : numbers.data(), numbers.size(), nr, column.data(), &sel, o.offsets.data(), o.valid.data(),
                     capacity, o.elements.get(), layout_only ? 0 : room, &o.res, &o.esel);
    return o;
}

}  // namespace

int main() {
    const char *pointers[] = {"/a", "", "/a/b"};
    std::vector<Paths> blob(1);
    if (sm_compile_paths(pointers, 3, blob.data(), nullptr) != 0) return fail("compile");
    const std::string stream =
        "{\"a\":[1,\"x\\n\",null,true,2.5,{\"b\":[7]}]} [[],[]] [{}] {\"a\":{\"b\":[[1,2],[3]]}} [] 7 {\"a\":[[[]],[],{\"a\":[]}]} [{\"a\":[1,2]},3]\n";
    unsigned seed = 4711;
    for (int round = 0; round < 400; round++) {
        std::string s = stream;
        if (round > 0)  // byte edits: whatever the arrays hold then, every access stays in bounds
            for (int e = 0; e < 1 + round % 3; e++) {
                seed = seed * 1103515245u + 12345u;
                s[(seed >> 8) % s.size()] = "{}[]:,\"\\u 1a"[(seed >> 20) % 12];
            }
        Tokens t = tokenize(s);
        const uint64_t n = t.idx.size(), D = t.first.size();
        msj_documents_result docs{D, D, n, s.size()};
        std::vector<msj_number> numbers;
        for (uint64_t i = 0; i < n; i++)
            if (t.flags[i] & 4) numbers.push_back(msj_number{(uint64_t)i, (uint32_t)i, (t.flags[i] & 8) ? 2u : 1u});
        msj_numbers_result nr{numbers.size(), 0, ~0ull, 0};
        std::vector<msj_field> fields(3 * D);
        msj_select_documents_result sel;
        sm_select_documents(blob.data(), (const uint8_t *)s.data(), s.size(), t.idx.data(), n, t.typ.data(), t.dep.data(), t.mat.data(),
                            t.end.data(), t.flags.data(), t.first.data(), &docs, numbers.empty() ? nullptr : numbers.data(), numbers.size(), &nr,
                            nullptr, fields.data(), D, &sel);
        for (int p = 0; p < 3; p++) {
            const std::vector<msj_field> column(fields.begin() + p * D, fields.begin() + (p + 1) * D);
            const Out layout = run(t, docs, numbers, round % 2 ? nullptr : &nr, column, sel, D, 0, true);
            const uint64_t total = layout.res.n_elements;
            if (layout.res.code != 0 || layout.offsets[D] != total) return fail("layout");
            for (uint64_t room : {total, total > 0 ? total - 1 : 0, (uint64_t)0}) {
                const Out o = run(t, docs, numbers, round % 2 ? nullptr : &nr, column, sel, D, room, false);
                if (o.res.n_elements != total || o.res.code != (total > room ? MSJ_CAPACITY : 0) || o.offsets != layout.offsets) return fail("clip");
            }
            if (D > 0 && run(t, docs, numbers, &nr, column, sel, D - 1, total, false).res.code != MSJ_CAPACITY) return fail("rows");
            // hostile records: every row's token moved about, tags forced to '[' -- in bounds whatever they name
            std::vector<msj_field> bad = column;
            for (uint64_t k = 0; k < D; k++) {
                seed = seed * 1103515245u + 12345u;
                const uint32_t pick = (seed >> 12) % 6;
                bad[k].code = 0, bad[k].type = '[';
                bad[k].token = pick == 0 ? (uint32_t)n : pick == 1 ? 0xFFFFFFFFu : pick == 2 ? (uint32_t)((seed >> 4) % (n + 1)) : pick == 3 ? t.first[(k + 1) % D] : column[k].token;
            }
            const Out h = run(t, docs, numbers, &nr, bad, sel, D, total, false);
            if (h.res.n_rows != D || h.offsets[D] != h.res.n_elements) return fail("hostile");
            if (round > 0) continue;
            const Out o = run(t, docs, numbers, &nr, column, sel, D, total, false);
            const uint64_t want_a[] = {0, 6, 6, 6, 6, 6, 6, 9, 9}, want_root[] = {0, 0, 2, 3, 3, 3, 3, 3, 5}, want_ab[] = {0, 0, 0, 0, 2, 2, 2, 2, 2};
            const uint64_t *want = p == 0 ? want_a : p == 1 ? want_root : want_ab;
            for (uint64_t k = 0; k <= D; k++)
                if (D != 8 || o.offsets[k] != want[k]) return fail("offsets");
            if (p == 0 && (o.elements[0].type != 'l' || o.elements[1].type != '"' || o.elements[1].flags != 2 || o.elements[4].type != 'd' ||
                           o.elements[5].type != '{' || o.elements[6].type != '[' || o.res.n_arrays != 2 || o.res.n_other != 1))
                return fail("/a");
            if (p == 1 && (o.elements[0].type != '[' || o.elements[2].type != '{' || o.res.n_arrays != 4 || o.res.n_other != 4)) return fail("root");
        }
    }
    printf("array_column_sanitize ok\n");
    return 0;
}
