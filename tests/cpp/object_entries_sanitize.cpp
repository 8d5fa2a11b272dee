// Test-only program (its own main): the host twin of msj_object_entries_device (tests/object_entries_math_host.cpp, and
// through it mojo_simdjson_amd/csrc/object_entries_math.h) under AddressSanitizer + UndefinedBehaviorSanitizer, fed by the
// select twin, the array-column twin and the select-elements twin.  tests/test_object_entries_sanitizers.py builds it with
// -fsanitize=address,undefined and runs it.  Every array is allocated at its exact size, so a read or a store one element
// out shows.  A small serial tokenizer below stands in for stage 1 + prep + split: it only has to give arrays of the right
// shape, also for the mutated inputs and the hostile records, where the call must stay in bounds whatever they hold.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../array_column_math_host.cpp"
#include "../object_entries_math_host.cpp"
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
    printf("object_entries_sanitize: %s\n", what);
    return 1;
}

struct Out {
    std::vector<uint64_t> offsets;
    std::vector<uint8_t> valid;
    std::vector<msj_field> keys, values;
    msj_object_entries_result res;
    msj_select_documents_result ksel, vsel;
};

// one call with every array at its exact size; room < 0: the layout-only form
Out run(const Tokens &t, const std::vector<msj_number> &numbers, const msj_numbers_result *nr, const std::vector<msj_field> &rows,
        const msj_select_documents_result &rows_select, uint64_t capacity, int64_t room) {
    Out o;
    o.offsets.resize(capacity + 1);
    o.valid.resize(capacity);
    if (room > 0) o.keys.resize((size_t)room), o.values.resize((size_t)room);
    oem_object_entries(t.idx.data(), t.idx.size(), t.typ.data(), t.dep.data(), t.mat.data(), t.end.data(), t.flags.data(),
                       numbers.empty() ? nullptr : numbers.data(), numbers.size(), nr, rows.empty() ? nullptr : rows.data(), &rows_select,
                       o.offsets.data(), o.valid.empty() ? nullptr : o.valid.data(), capacity, o.keys.empty() ? nullptr : o.keys.data(),
                       o.values.empty() ? nullptr : o.values.data(), room > 0 ? (uint64_t)room : 0, &o.res, &o.ksel, &o.vsel);
    return o;
}
// the layout-only form, then the complete column
Out complete(const Tokens &t, const std::vector<msj_number> &numbers, const msj_numbers_result *nr, const std::vector<msj_field> &rows,
             const msj_select_documents_result &rows_select) {
    const Out lay = run(t, numbers, nr, rows, rows_select, rows.size(), -1);
    return run(t, numbers, nr, rows, rows_select, rows.size(), (int64_t)lay.res.n_entries);
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
msj_field coded_record(uint16_t code) {
    msj_field f{};
    f.token = 0xFFFFFFFFu, f.code = code;
    return f;
}

// the hostile records of one window: ascending tokens from anywhere in [0, n + 2] and past it, every one claiming an object,
// records with a code between them; a swapped and an equal pair; every token a row; partners moved; a row inside a row
int hostile(const Tokens &t, const std::vector<msj_number> &numbers, const msj_numbers_result *nrp, const std::vector<msj_field> &rows,
            const msj_select_documents_result &rsel, unsigned &seed) {
    const uint64_t n = t.idx.size(), R = rows.size();
    std::vector<uint32_t> picks;
    for (uint64_t k = 0; k < R + 3; k++) {
        seed = seed * 1103515245u + 12345u;
        picks.push_back((seed >> 12) % 9 == 0 ? 0xFFFFFFF0u + (uint32_t)k : (uint32_t)((seed >> 4) % (n + 3)));
    }
    std::sort(picks.begin(), picks.end());
    picks.erase(std::unique(picks.begin(), picks.end()), picks.end());
    std::vector<msj_field> bad;
    std::vector<size_t> live;
    for (uint32_t v : picks) {
        seed = seed * 1103515245u + 12345u;
        for (unsigned c = (seed >> 9) % 3; c > 0; c--) bad.push_back(coded_record(c == 1 ? 20 : 17));
        live.push_back(bad.size());
        bad.push_back(object_record(v));
    }
    bad.push_back(coded_record(20));
    const Out h = complete(t, numbers, nrp, bad, select_result(bad.size()));
    if (h.res.code != 0 || h.res.n_rows != bad.size()) return fail("hostile");
    if (live.size() > 1) {
        std::swap(bad[live.front()], bad[live.back()]);
        const Out x = run(t, numbers, nrp, bad, select_result(bad.size()), bad.size(), 4);
        if (x.res.code != MSJ_ERR_BAD_ARGUMENT || x.res.n_rows != bad.size() || x.res.n_objects != 0 || x.ksel.n_documents != 0) return fail("order");
        bad[live.back()] = bad[live.front()];  // an equal pair
        if (live.size() > 2 && run(t, numbers, nrp, bad, select_result(bad.size()), bad.size(), 4).res.code != MSJ_ERR_BAD_ARGUMENT)
            return fail("equal");
    }
    // every token a row (rows inside rows, rows whose own token is a key), and the partners moved about under true rows
    std::vector<msj_field> all;
    for (uint64_t v = 0; v < n; v++) all.push_back(object_record((uint32_t)v));
    if (complete(t, numbers, nrp, all, select_result(n)).res.n_rows != n) return fail("all");
    Tokens u = t;
    for (uint64_t v = 0; v < n; v++) {
        seed = seed * 1103515245u + 12345u;
        if ((seed >> 10) % 4 == 0) u.mat[v] = (seed >> 14) % 3 == 0 ? msj::tape::kNoPartner : (uint32_t)((seed >> 4) % (n + 2));
    }
    if (complete(u, numbers, nrp, rows, rsel).res.n_rows != R) return fail("partners");
    if (complete(u, numbers, nrp, all, select_result(n)).res.n_rows != n) return fail("partners under every token");
    return 0;
}

}  // namespace

int main() {
    const char *doc_pointers[] = {"/attrs", "/items", ""};
    const char *dims_pointer[] = {"/dims"};
    std::vector<msj::sel::Paths> docs_paths(1), dims(1);
    if (sm_compile_paths(doc_pointers, 3, docs_paths.data(), nullptr) != 0 || sm_compile_paths(dims_pointer, 1, dims.data(), nullptr) != 0)
        return fail("compile");
    const std::string stream =
        "{\"attrs\":{\"color\":\"red\",\"size\":\"L\",\"n\":{\"deep\":1,\"m\":{\"x\":2}}},\"items\":[{\"sku\":1,\"dims\":{\"w\":1,\"h\":2.5}},{\"sku\":2},7,"
        "{\"dims\":{\"d\":{\"e\":9},\"d\":3}}]} {\"a\\n\":1,\"\":[{\"b\":2}],\"c\":{}} "
        "{\"attrs\":{},\"items\":[]} {\"attrs\":7,\"items\":[{\"dims\":[1]},{\"dims\":{\"k\":\"v\"}}]} {\"a\":} {\"a\":,\"b\":1} {\"a\" \"b\":1} []\n";
    unsigned seed = 7013;
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
        std::vector<msj_field> columns(3 * D);
        msj_select_documents_result sel;
        sm_select_documents(docs_paths.data(), (const uint8_t *)s.data(), s.size(), t.idx.data(), n, t.typ.data(), t.dep.data(), t.mat.data(),
                            t.end.data(), t.flags.data(), t.first.data(), &docs, numbers.empty() ? nullptr : numbers.data(), numbers.size(), &nr,
                            nullptr, columns.data(), D, &sel);
        for (int p = 0; p < 3; p++) {
            // source 1: the documents as the rows, one path's column; then the call over its own values, two more levels
            const std::vector<msj_field> column(columns.begin() + p * D, columns.begin() + (p + 1) * D);
            msj_select_documents_result csel = sel;
            csel.n_paths = 1;
            const Out o = complete(t, numbers, nrp, column, csel);
            if (o.res.code != 0 || o.res.n_rows != D || o.ksel.n_documents != o.res.n_entries || o.vsel.n_no_bits != o.res.n_no_bits) return fail("call");
            uint64_t objects = 0;
            for (uint8_t v : o.valid) objects += v;
            if (objects != o.res.n_objects || o.offsets[D] != o.res.n_entries || o.ksel.n_no_bits != 0) return fail("counts");
            for (uint64_t e = 0; e < o.res.n_entries; e++)
                if (o.keys[e].token + 2 != o.values[e].token || o.keys[e].type != '"') return fail("pairs");
            const Out o2 = complete(t, numbers, nrp, o.values, o.vsel);   // (value records ascend: token order)
            const Out o3 = complete(t, numbers, nrp, o2.values, o2.vsel);
            if (o2.res.code != 0 || o3.res.code != 0 || o3.res.n_rows != o2.res.n_entries) return fail("levels");
            if (D > 0 && run(t, numbers, nrp, column, csel, D - 1, 4).res.code != MSJ_CAPACITY) return fail("capacity");
            if (o.res.n_entries > 1) {  // (room 0 would be the layout-only form)
                const Out clip = run(t, numbers, nrp, column, csel, D, (int64_t)o.res.n_entries - 1);
                if (clip.res.code != MSJ_CAPACITY || clip.res.n_entries != o.res.n_entries || clip.offsets != o.offsets) return fail("clipped entries");
                if (run(t, numbers, nrp, column, csel, D, 1).res.n_entries != o.res.n_entries) return fail("one entry");
            }
            if (run(t, numbers, nrp, column, select_result(D, MSJ_CAPACITY), D, 4).res.n_rows != 0) return fail("clipped rows");
            if (hostile(t, numbers, nrp, column, csel, seed)) return 1;
            // source 2: the elements of the path's arrays as the rows; source 3: /dims looked up in them
            std::vector<uint64_t> offsets(D + 1);
            std::vector<uint8_t> valid(D);
            msj_array_column_result ares;
            msj_select_documents_result psel;
            acm_array_column(t.idx.data(), n, t.typ.data(), t.dep.data(), t.mat.data(), t.end.data(), t.flags.data(), t.first.data(), &docs,
                             numbers.empty() ? nullptr : numbers.data(), numbers.size(), &nr, column.data(), &csel, offsets.data(), valid.data(), D,
                             nullptr, 0, &ares, nullptr);
            const uint64_t R = ares.n_elements;
            std::vector<msj_field> rows(R);
            acm_array_column(t.idx.data(), n, t.typ.data(), t.dep.data(), t.mat.data(), t.end.data(), t.flags.data(), t.first.data(), &docs,
                             numbers.empty() ? nullptr : numbers.data(), numbers.size(), &nr, column.data(), &csel, offsets.data(), valid.data(), D,
                             rows.empty() ? nullptr : rows.data(), R, &ares, &psel);
            if (psel.code != 0 || psel.n_documents != R) return fail("rows");
            const Out e = complete(t, numbers, nrp, rows, psel);
            if (e.res.code != 0 || e.res.n_rows != R) return fail("elements");
            std::vector<msj_field> fields(R);
            msj_select_documents_result fsel;
            sem_select_elements(dims.data(), (const uint8_t *)s.data(), s.size(), t.idx.data(), n, t.typ.data(), t.dep.data(), t.mat.data(),
                                t.end.data(), t.flags.data(), numbers.empty() ? nullptr : numbers.data(), numbers.size(), nrp,
                                rows.empty() ? nullptr : rows.data(), &psel, fields.empty() ? nullptr : fields.data(), R, &fsel);
            const Out g = complete(t, numbers, nrp, fields, fsel);
            if (g.res.code != 0 || g.res.n_rows != R) return fail("dims");
            if (hostile(t, numbers, nrp, fields, fsel, seed)) return 1;
            if (round > 0) continue;
            if (p == 0) {  // /attrs: {color,size,n} -- 20 -- {} -- 7 -- 20 x 4
                const uint64_t want[] = {0, 3, 3, 3, 3, 3, 3, 3, 3};
                if (D != 8 || o.res.n_objects != 2 || o.res.n_other != 1 || !std::equal(want, want + 9, o.offsets.begin())) return fail("/attrs");
                if (o.values[0].type != '"' || o.values[2].type != '{' || o2.res.n_objects != 1 || o2.res.n_entries != 2 || o3.res.n_entries != 1)
                    return fail("map of maps");
            } else if (p == 1) {  // /items: four elements, then none, then two
                const uint64_t want[] = {0, 2, 2, 2, 4, 4, 5};
                if (R != 6 || e.res.n_objects != 5 || e.res.n_other != 1) return fail("/items");
                if (fields[0].code != 0 || fields[1].code != 20 || fields[2].code != 17 || fields[3].code != 0) return fail("codes");
                if (g.res.n_objects != 3 || g.res.n_other != 1 || !std::equal(want, want + 7, g.offsets.begin())) return fail("/items/dims");
                if (g.values[1].type != 'd' || g.values[2].type != '{' || g.values[3].type != 'l' || g.keys[2].token == g.keys[3].token) return fail("duplicates");
            } else {  // the documents themselves: the second one has an escaped key, the empty key and {}
                if (o.res.n_objects != 7 || o.res.n_other != 1) return fail("root");
                if (o.offsets[1] != 2 || o.offsets[2] != 5 || (o.keys[2].flags & 2) == 0 || (o.keys[3].bits >> 32) != 0) return fail("root keys");
                // {"a":} {"a":,"b":1} {"a" "b":1}: none; ("a", ',') and ("b", 1); ("b", 1)
                if (o.offsets[5] - o.offsets[4] != 0 || o.offsets[6] - o.offsets[5] != 2 || o.offsets[7] - o.offsets[6] != 1) return fail("malformed");
                if (o.values[o.offsets[5]].type != ',' || o.values[o.offsets[6]].type != 'l') return fail("malformed values");
            }
        }
    }
    printf("object_entries_sanitize ok\n");
    return 0;
}
