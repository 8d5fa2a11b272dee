// Stand-alone program (its own main; built by tests/test_dictionary_extend_sanitizers.py with -fsanitize=address,undefined):
// the host form of msj_dictionary_extend_device's arithmetic (tests/dictionary_extend_math_host.cpp over
// csrc/dictionary_extend_math.h) on arrays from anywhere.  A pinned chain -- three windows of repeated values, "", null rows,
// prefixes and values of some thousand bytes into one dictionary -- and then, round after round, damaged copies: row offsets
// and valid bytes as tests/cpp/dictionary_sanitize.cpp damages them, prior offsets that descend, lie past
// dict_bytes_capacity or are huge, a P below, at and above dict_capacity, a row count above `rows`.  Every array is a
// std::vector of exactly its size, so a read or a write outside is the sanitizer's to report.  Asserted here: nothing of
// the prior part and nothing past a capacity is written, the codes are -1, -2 (frozen only), a prior entry of the same bytes
// or a new code whose first row has the same bytes, and both hashes and both orders of insertion give the same codes.  NOT
// part of the product.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../dictionary_extend_math_host.cpp"

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
constexpr uint64_t kFill64 = 0x7777777777777777ull;

struct Column {
    std::vector<uint64_t> offsets;
    std::vector<uint8_t> valid, bytes;
};
struct Dict {  // dict_capacity + 1 offsets, dict_capacity first rows, dict_bytes_capacity bytes
    std::vector<uint64_t> offsets;
    std::vector<uint32_t> first;
    std::vector<uint8_t> bytes;
};

// One call into a copy of `d` with P prior entries; what it may not touch is compared with `d` -> the codes
std::vector<int32_t> run(const Column &c, uint64_t bytes_len, const uint64_t *n_rows, const Dict &d, uint64_t P, uint32_t flags, int order,
                         Dict *left = nullptr, uint64_t *n_distinct = nullptr) {
    const uint64_t rows = c.valid.size(), cap = d.first.size(), room = d.bytes.size();
    Dict out = d;
    std::vector<int32_t> codes(rows, 0x77777777);
    msj_dictionary_extend_result res;
    dxm_dictionary_extend(c.offsets.data(), c.valid.data(), rows, n_rows, c.bytes.data(), bytes_len, 0, &P, codes.data(), out.offsets.data(),
                          out.first.data(), cap, out.bytes.data(), room, flags, order, &res);
    const uint64_t R = n_rows ? *n_rows : rows;
    const bool frozen = (flags & MSJ_DICTIONARY_FROZEN) != 0;
    CHECK(res.n_rows == R && res.flags == flags && res.n_prior == P);
    bool over = R > rows || R >= (1ull << 31) || P > cap || P + R >= (1ull << 31);
    if (!over) over = (P ? d.offsets[P] : 0) > room;
    if (over || frozen) {
        CHECK(out.offsets == d.offsets && out.first == d.first && out.bytes == d.bytes);
        CHECK(res.code == (over ? MSJ_CAPACITY : 0));
        if (over) {
            CHECK(res.n_values == 0 && res.n_distinct == 0 && res.dict_bytes == 0 && res.n_matched == 0);
            for (int32_t x : codes) CHECK(x == 0x77777777);
            return codes;
        }
    }
    const uint64_t base = P ? d.offsets[P] : 0;
    const Source src{c.offsets.data(), c.valid.data(), c.bytes.data(), bytes_len, d.offsets.data(), d.bytes.data(), room};
    // the prior part, and what lies past the entries and the bytes the result names
    for (uint64_t e = P ? 0 : 1; e <= P && e <= cap; e++) CHECK(out.offsets[e] == d.offsets[e]);
    for (uint64_t e = 0; e < P; e++) CHECK(out.first[e] == d.first[e]);
    for (uint64_t b = 0; b < base; b++) CHECK(out.bytes[b] == d.bytes[b]);
    for (uint64_t e = res.n_distinct; e < cap; e++) CHECK(out.first[e] == d.first[e] && out.offsets[e + 1] == d.offsets[e + 1]);
    for (uint64_t b = res.dict_bytes; b < room; b++) CHECK(out.bytes[b] == d.bytes[b]);
    CHECK(res.n_distinct >= P && res.dict_bytes >= base && res.n_matched <= res.n_values && res.n_values <= R);
    if (!frozen) CHECK(res.code == (res.n_distinct > cap || res.dict_bytes > room ? MSJ_CAPACITY : 0));
    if (!frozen && P == 0) CHECK(out.offsets[0] == 0);
    uint64_t values = 0, matched = 0;
    for (uint64_t k = 0; k < rows; k++) {
        if (k >= R) {
            CHECK(codes[k] == 0x77777777);
            continue;
        }
        const Item y = item_of(src, P, P + k);
        CHECK((codes[k] == -1) == !y.has);
        if (!y.has) continue;
        values++;
        if (codes[k] == kNoEntry) {
            CHECK(frozen);
            continue;
        }
        CHECK(codes[k] >= 0 && (uint64_t)codes[k] < res.n_distinct);
        if ((uint64_t)codes[k] < P) {  // a prior entry of the same bytes, and no lower one
            matched++;
            const Item z = prior_of(src, codes[k]);
            CHECK(z.has && z.len == y.len && (y.len == 0 || memcmp(z.p, y.p, y.len) == 0));
            continue;
        }
        CHECK(!frozen);
        if ((uint64_t)codes[k] >= cap) continue;
        const uint32_t f = out.first[codes[k]];
        CHECK(f <= k && codes[f] == codes[k]);
        const Item z = item_of(src, P, P + f);
        CHECK(z.has && z.len == y.len && (y.len == 0 || memcmp(z.p, y.p, y.len) == 0));
        CHECK(out.offsets[codes[k] + 1] - out.offsets[codes[k]] == y.len);
        for (uint64_t b = 0; b < y.len && out.offsets[codes[k]] + b < room; b++) CHECK(out.bytes[out.offsets[codes[k]] + b] == y.p[b]);
    }
    CHECK(values == res.n_values && matched == res.n_matched);
    if (left) *left = out;
    if (n_distinct) *n_distinct = res.n_distinct;
    return codes;
}

// the prior part of `prior` in arrays with room for so many more entries and bytes, each at its exact size
Dict with_room(const Dict &prior, uint64_t P, uint64_t more_entries, uint64_t more_bytes) {
    Dict d;
    const uint64_t base = P ? prior.offsets[P] : 0, kept = base <= prior.bytes.size() ? base : prior.bytes.size();
    d.offsets.assign(P + more_entries + 1, kFill64), d.first.assign(P + more_entries, 0x77777777u), d.bytes.assign(kept + more_bytes, kFill);
    for (uint64_t e = 0; e <= P && e < prior.offsets.size(); e++) d.offsets[e] = prior.offsets[e];
    for (uint64_t b = 0; b < kept; b++) d.bytes[b] = prior.bytes[b];
    return d;
}

// with room for everything, for one more entry, for one more byte, for nothing more.  (The room is part of the input: a
// damaged prior entry has a value only below dict_bytes_capacity, so the codes are compared form by form)
void all_forms(const Column &c, uint64_t bytes_len, const uint64_t *n_rows, const Dict &prior, uint64_t P) {
    const Dict forms[] = {with_room(prior, P, c.valid.size(), bytes_len), with_room(prior, P, 1, bytes_len), with_room(prior, P, c.valid.size(), 1),
                          with_room(prior, P, 0, 0)};
    for (const Dict &d : forms) {
        const std::vector<int32_t> want = run(c, bytes_len, n_rows, d, P, 0, 0);
        const std::vector<int32_t> frozen = run(c, bytes_len, n_rows, d, P, MSJ_DICTIONARY_FROZEN, 0);
        for (uint32_t flags = 0; flags < 4; flags++)
            for (int order = 0; order < 2; order++) CHECK(run(c, bytes_len, n_rows, d, P, flags, order) == (flags & MSJ_DICTIONARY_FROZEN ? frozen : want));
    }
}

Column window(int round) {
    Column c;
    c.offsets.push_back(0);
    const std::string big(3000, 'z');
    const std::string values[] = {"red", "green", "", "red", "re", "redd", big, "blue", "", big, big.substr(0, 2999) + "y", "green"};
    for (int j = 0; j < 12; j++) {
        const std::string v = round == 2 && j % 4 == 1 ? values[j] + "-late" : values[(j + 5 * round) % 12];
        c.bytes.insert(c.bytes.end(), v.begin(), v.end());
        c.offsets.push_back(c.bytes.size());
        c.valid.push_back(1);
        if (round == 1) c.offsets.push_back(c.bytes.size()), c.valid.push_back(0);  // a null row behind each
    }
    return c;
}

}  // namespace

int main() {
    // the pinned chain: three windows into one dictionary, each call's P the previous n_distinct
    Dict chain = with_room(Dict{{0}, {}, {}}, 0, 40, 16000);
    uint64_t P = 0;
    std::vector<Dict> stages{chain};
    std::vector<uint64_t> priors{0};
    for (int round = 0; round < 3; round++) {
        const Column c = window(round);
        all_forms(c, c.bytes.size(), nullptr, chain, P);
        Dict left;
        run(c, c.bytes.size(), nullptr, chain, P, 0, 0, &left, &P);
        chain = left;
        stages.push_back(chain), priors.push_back(P);
    }
    CHECK(P == 11);  // red green "" re redd big blue big-y; the second window adds none; green-late redd-late big-late
    const Column pin = window(2);
    const uint64_t rows = pin.valid.size(), len = pin.bytes.size();
    for (uint64_t r : std::vector<uint64_t>{0, 1, rows - 1, rows, rows + 1, ~(uint64_t)0}) all_forms(pin, len, &r, stages[2], priors[2]);
    for (uint64_t p : std::vector<uint64_t>{0, 1, priors[2] - 1, 40, 41, 1ull << 31, ~(uint64_t)0}) {
        run(pin, len, nullptr, stages[2], p, 0, 0);
        run(pin, len, nullptr, stages[2], p, MSJ_DICTIONARY_FROZEN, 1);
    }
    all_forms(Column{{0}, {}, {}}, 0, nullptr, stages[2], priors[2]);
    for (int round = 0; round < 300; round++) {
        Column c = window(round % 3);
        Dict d = stages[2];
        const uint64_t p = priors[2], c_len = c.bytes.size();
        const int hits = 1 + (int)(rnd() % 6);
        for (int j = 0; j < hits; j++) {
            const uint64_t k = rnd() % c.offsets.size(), e = rnd() % (p + 1);
            switch (rnd() % 8) {
                case 0: c.offsets[k] = rnd() % (c_len + 3); break;
                case 1: c.offsets[k] = rnd(); break;
                case 2: c.valid[rnd() % c.valid.size()] = (uint8_t)rnd(); break;
                case 3: c.offsets[k] = k ? c.offsets[k - 1] - (k > 1 && c.offsets[k - 1] ? 1 : 0) : 0; break;
                case 4: d.offsets[e] = rnd() % (d.offsets[p] + 3); break;
                case 5: d.offsets[e] = rnd(); break;
                case 6: d.offsets[e] = d.bytes.size() + 1 + rnd() % 5; break;
                default: d.offsets[e] = e ? d.offsets[e - 1] : 0; break;  // a duplicate of "" or an entry that swallows its neighbour
            }
        }
        uint64_t short_len = c_len;
        if (round % 3 == 0) {  // a window of bytes shorter than the offsets say, at its exact size
            short_len = rnd() % (c_len + 1);
            c.bytes.resize(short_len);
            c.bytes.shrink_to_fit();
        }
        all_forms(c, short_len, nullptr, d, p);
        if (round % 7 == 0) {
            const uint64_t r = rnd() % (c.valid.size() + 2);
            all_forms(c, short_len, &r, d, p);
        }
    }
    if (failures) return 1;
    printf("dictionary_extend_sanitize ok\n");
    return 0;
}
