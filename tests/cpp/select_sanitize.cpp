// Test-only program (its own main): the host twin of msj_select_documents_device (tests/select_math_host.cpp, and through it
// mojo_simdjson_amd/csrc/select_math.h) under AddressSanitizer + UndefinedBehaviorSanitizer.  tests/test_select_sanitizers.py
// builds it with -fsanitize=address,undefined and runs it.  Every array is allocated at its exact size, so a read or a store
// one element out shows.  A small serial tokenizer below stands in for stage 1 + prep + split: it only has to give arrays of
// the right shape, also for the mutated inputs, where the lookup must stay in bounds whatever they hold.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

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
    printf("select_sanitize: %s\n", what);
    return 1;
}

}  // namespace

int main() {
    const char *pointers[] = {"/a", "/a/b", "", "/k\\u/x", "/n", "/~0~1"};
    std::vector<Paths> blob(1);
    uint32_t levels[16];
    if (sm_compile_paths(pointers, 6, blob.data(), levels) != 0 || levels[1] != 2 || levels[2] != 0) return fail("compile");
    const char *bad[] = {"/a", "b"};
    if (sm_compile_paths(bad, 2, blob.data(), nullptr) != 22 || sm_compile_paths(pointers, 17, blob.data(), nullptr) != -1) return fail("refuse");
    std::string seg(256, 'k');
    seg[0] = '/';
    const char *longest[] = {seg.c_str()};
    if (sm_compile_paths(longest, 1, blob.data(), levels) != 0) return fail("255 bytes");
    seg += "k";
    const char *too_long[] = {seg.c_str()};
    if (sm_compile_paths(too_long, 1, blob.data(), levels) != -1) return fail("256 bytes");
    if (sm_compile_paths(pointers, 6, blob.data(), levels) != 0) return fail("compile again");

    const std::string stream =
        "{\"a\":1,\"a\":2} {\"x\":{\"a\":1},\"a\":{\"b\":\"v\\n\"}} [1,{\"a\":2}] \"s\" -2.5 {\"\\u0061\":{\"b\":[1,2]},\"n\":null,\"~/\":true}\n";
    unsigned seed = 12345;
    for (int round = 0; round < 400; round++) {
        std::string s = stream;
        if (round > 0)  // byte edits: whatever the arrays hold then, every access stays in bounds
            for (int e = 0; e < 1 + round % 3; e++) {
                seed = seed * 1103515245u + 12345u;
                s[(seed >> 8) % s.size()] = "{}[]:,\"\\u 1a"[(seed >> 20) % 12];
            }
        Tokens t = tokenize(s);
        const uint64_t n = t.idx.size();
        msj_documents_result docs{t.first.size(), t.first.size(), n, s.size()};
        std::vector<msj_number> numbers;
        for (uint64_t i = 0; i < n; i++)
            if (t.flags[i] & 4) numbers.push_back(msj_number{(uint64_t)i, (uint32_t)i, (t.flags[i] & 8) ? 2u : 1u});
        msj_numbers_result nr{numbers.size(), 0, ~0ull, 0};
        const uint64_t D = t.first.size();
        for (uint64_t capacity : {D, D > 0 ? D - 1 : 0}) {
            std::vector<msj_field> fields(6 * capacity);
            msj_select_documents_result res;
            sm_select_documents(blob.data(), (const uint8_t *)s.data(), s.size(), t.idx.data(), n, t.typ.data(), t.dep.data(), t.mat.data(),
                                t.end.data(), t.flags.data(), t.first.data(), &docs, numbers.empty() ? nullptr : numbers.data(), numbers.size(),
                                round % 2 ? nullptr : &nr, nullptr, fields.data(), capacity, &res);
            if (round > 0 || capacity != D) continue;
            if (res.code != 0 || res.n_documents != 6 || res.n_paths != 6) return fail("result");
            auto at = [&](int p, int k) { return fields[p * capacity + k]; };
            if (at(0, 0).type != 'l' || at(0, 0).bits != at(0, 0).token || at(0, 0).code != 0) return fail("first duplicate");
            if (at(1, 1).type != '"' || at(1, 1).flags != 2 || (at(1, 1).bits >> 32) != 3) return fail("/a/b");
            if (at(0, 2).code != 17 || at(0, 3).code != 17 || at(2, 4).type != 'd') return fail("no object");
            if (at(0, 5).type != '{' || at(1, 5).type != '[' || at(4, 5).type != 'n' || at(5, 5).type != 't') return fail("escaped key");
            if (at(3, 5).code != 20 || at(4, 0).code != 20) return fail("no such field");
        }
    }
    printf("select_sanitize ok\n");
    return 0;
}
