// Test-only program (its own main): the host twin of msj_select_elements_device (tests/select_elements_math_host.cpp, and
// through it mojo_simdjson_amd/csrc/select_elements_math.h) under AddressSanitizer + UndefinedBehaviorSanitizer, fed by the
// select twin and the array-column twin.  tests/test_select_elements_sanitizers.py builds it with
// -fsanitize=address,undefined and runs it.  Every array is allocated at its exact size, so a read or a store one element
// out shows.  A small serial tokenizer below stands in for stage 1 + prep + split: it only has to give arrays of the right
// shape, also for the mutated inputs and the hostile records, where the call must stay in bounds whatever they hold.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../array_column_math_host.cpp"
#include "../select_elements_math_host.cpp"
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
        uint32_t e = 0, m = msj::tape::kNoPartner;
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
    printf("select_elements_sanitize: %s\n", what);
    return 1;
}

struct Out {
    std::vector<msj_field> fields;
    msj_select_documents_result res;
};

// one call with every array at its exact size
Out run(const std::vector<msj::sel::Paths> &blob, const std::string &s, const Tokens &t, const std::vector<msj_number> &numbers,
        const msj_numbers_result *nr, const std::vector<msj_field> &rows, const msj_select_documents_result &rows_select, uint64_t capacity) {
    Out o;
    o.fields.resize(blob[0].n_paths * capacity);
    sem_select_elements(blob.data(), (const uint8_t *)s.data(), s.size(), t.idx.data(), t.idx.size(), t.typ.data(), t.dep.data(), t.mat.data(),
                        t.end.data(), t.flags.data(), numbers.empty() ? nullptr : numbers.data(), numbers.size(), nr,
                        rows.empty() ? nullptr : rows.data(), &rows_select, o.fields.empty() ? nullptr : o.fields.data(), capacity, &o.res);
    return o;
}

msj_select_documents_result select_result(uint64_t rows, int32_t code = 0) {
    msj_select_documents_result r{};
    r.code = code, r.n_documents = r.n_found = rows, r.n_paths = 1;
    return r;
}

msj_field object_record(uint32_t token) {
    msj_field f{};
    f.token = token, f.type = '{';
    return f;
}

}  // namespace

int main() {
    const char *list_pointers[] = {"/items", ""};
    const char *pointers[] = {"/sku", "/qty", "/dims/w", ""};
    std::vector<msj::sel::Paths> lists(1), blob(1);
    if (sm_compile_paths(list_pointers, 2, lists.data(), nullptr) != 0 || sm_compile_paths(pointers, 4, blob.data(), nullptr) != 0)
        return fail("compile");
    const std::string stream =
        "{\"items\":[{\"sku\":\"a\",\"qty\":2},{\"qty\":3},7,\"s\",[],{},null]} [{\"x\":{\"sku\":1},\"sku\":2}] "
        "{\"items\":[{\"s\\u006bu\":\"e\\nv\",\"dims\":{\"w\":1.5}},{\"dims\":5},{\"dims\":{\"h\":2}}]} [{\"a\":[{\"sku\":9}]},{\"sku\":1,\"sku\":3}] {\"items\":7} []\n";
    unsigned seed = 4712;
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
        const msj_numbers_result *nrp = round % 2 ? nullptr : &nr;
        std::vector<msj_field> columns(2 * D);
        msj_select_documents_result sel;
        sm_select_documents(lists.data(), (const uint8_t *)s.data(), s.size(), t.idx.data(), n, t.typ.data(), t.dep.data(), t.mat.data(),
                            t.end.data(), t.flags.data(), t.first.data(), &docs, numbers.empty() ? nullptr : numbers.data(), numbers.size(), &nr,
                            nullptr, columns.data(), D, &sel);
        for (int p = 0; p < 2; p++) {
            const std::vector<msj_field> column(columns.begin() + p * D, columns.begin() + (p + 1) * D);
            std::vector<uint64_t> offsets(D + 1);
            std::vector<uint8_t> valid(D);
            msj_array_column_result ares;
            msj_select_documents_result esel;
            acm_array_column(t.idx.data(), n, t.typ.data(), t.dep.data(), t.mat.data(), t.end.data(), t.flags.data(), t.first.data(), &docs,
                             numbers.empty() ? nullptr : numbers.data(), numbers.size(), &nr, column.data(), &sel, offsets.data(), valid.data(), D,
                             nullptr, 0, &ares, nullptr);
            const uint64_t R = ares.n_elements;
            std::vector<msj_field> rows(R);
            acm_array_column(t.idx.data(), n, t.typ.data(), t.dep.data(), t.mat.data(), t.end.data(), t.flags.data(), t.first.data(), &docs,
                             numbers.empty() ? nullptr : numbers.data(), numbers.size(), &nr, column.data(), &sel, offsets.data(), valid.data(), D,
                             rows.empty() ? nullptr : rows.data(), R, &ares, &esel);
            if (esel.code != 0 || esel.n_documents != R) return fail("rows");
            const Out o = run(blob, s, t, numbers, nrp, rows, esel, R);
            if (o.res.code != 0 || o.res.n_documents != R || o.res.n_paths != 4) return fail("call");  // (element records always ascend)
            uint64_t found = 0;
            for (const msj_field &f : o.fields) found += f.code == 0;
            if (found != o.res.n_found) return fail("n_found");
            if (R > 0 && run(blob, s, t, numbers, nrp, rows, esel, R - 1).res.code != MSJ_CAPACITY) return fail("capacity");
            if (run(blob, s, t, numbers, nrp, rows, select_result(R, MSJ_CAPACITY), R).res.n_documents != 0) return fail("clipped");
            // hostile records: ascending tokens from anywhere in [0, n + 2] and past it, every one claiming an object; then
            // the same rows shuffled, which the order test refuses
            std::vector<uint32_t> picks;
            for (uint64_t k = 0; k < R + 3; k++) {
                seed = seed * 1103515245u + 12345u;
                picks.push_back((seed >> 12) % 9 == 0 ? 0xFFFFFFF0u + (uint32_t)k : (uint32_t)((seed >> 4) % (n + 3)));
            }
            std::sort(picks.begin(), picks.end());
            picks.erase(std::unique(picks.begin(), picks.end()), picks.end());
            std::vector<msj_field> bad;
            for (uint32_t v : picks) bad.push_back(object_record(v));
            const Out h = run(blob, s, t, numbers, nrp, bad, select_result(bad.size()), bad.size());
            if (h.res.code != 0 || h.res.n_documents != bad.size()) return fail("hostile");
            if (bad.size() > 1) {
                std::swap(bad[0], bad[bad.size() - 1]);
                if (run(blob, s, t, numbers, nrp, bad, select_result(bad.size()), bad.size()).res.code != MSJ_ERR_BAD_ARGUMENT) return fail("order");
            }
            // every token a row, and the partners moved about under true rows
            std::vector<msj_field> all;
            for (uint64_t v = 0; v < n; v++) all.push_back(object_record((uint32_t)v));
            if (run(blob, s, t, numbers, nrp, all, select_result(n), n).res.n_documents != n) return fail("all");
            Tokens u = t;
            for (uint64_t v = 0; v < n; v++) {
                seed = seed * 1103515245u + 12345u;
                if ((seed >> 10) % 4 == 0) u.mat[v] = (seed >> 14) % 3 == 0 ? msj::tape::kNoPartner : (uint32_t)((seed >> 4) % (n + 2));
            }
            if (run(blob, s, u, numbers, nrp, rows, esel, R).res.n_documents != R) return fail("partners");
            if (round > 0) continue;
            if (p == 0) {  // the lists at /items: 7 + 3 rows
                if (R != 10 || o.res.n_found != 2 + 2 + 1 + 10) return fail("/items");
                const msj_field *sku = o.fields.data(), *qty = sku + R, *w = qty + R, *self = w + R;
                const uint16_t want_sku[] = {0, 20, 17, 17, 17, 20, 17, 0, 20, 20}, want_w[] = {20, 20, 17, 17, 17, 20, 17, 0, 17, 20};
                for (uint64_t r = 0; r < R; r++)
                    if (sku[r].code != want_sku[r] || w[r].code != want_w[r] || self[r].code != 0) return fail("codes");
                if (sku[0].type != '"' || sku[7].flags != 2 || qty[0].type != 'l' || qty[0].bits != qty[0].token || w[7].type != 'd') return fail("values");
            } else {  // the documents that are arrays: 1 + 2 + 0 rows
                const msj_field *sku = o.fields.data();
                if (R != 3 || sku[0].code != 0 || sku[0].type != 'l' || sku[1].code != 20 || sku[2].code != 0) return fail("root");
                if (sku[0].token != sku[0].bits || t.idx[sku[0].token] != stream.find("2}]")) return fail("depth");  // not the deeper "sku":1
            }
        }
    }
    printf("select_elements_sanitize ok\n");
    return 0;
}
