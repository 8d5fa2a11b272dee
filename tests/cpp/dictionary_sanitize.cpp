// Stand-alone program (its own main; built by tests/test_dictionary_sanitizers.py with -fsanitize=address,undefined): the
// host form of msj_dictionary_device's arithmetic (tests/dictionary_math_host.cpp over csrc/dictionary_math.h) on arrays from
// anywhere.  A pinned column -- repeated values, "", null rows, prefixes, a value of some thousand bytes -- and then, round
// after round, damaged copies of its offsets and valid arrays: offsets that descend, lie past bytes_len, are huge; valid
// bytes from a generator; a bytes_len shorter than the offsets say; a row count on the device below and above `rows`.
// Every array is a std::vector of exactly its size, so a read or a write outside is the sanitizer's to report.  Asserted
// here: the counts add up, the codes are -1 or below n_distinct and name a first row of the same bytes, the dictionary
// offsets ascend by the values' lengths, nothing past the capacities is written, and both hashes and both orders of
// insertion give the same codes.  NOT part of the product.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../dictionary_math_host.cpp"

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

struct Column {
    std::vector<uint64_t> offsets;
    std::vector<uint8_t> valid, bytes;
};

// form 0: room for everything, 1: entries one short, 2: bytes one short, 3: layout-only, 4: no room at all
std::vector<int32_t> run(const Column &c, uint64_t bytes_len, const uint64_t *n_rows, uint32_t flags, int order, int form) {
    const uint64_t rows = c.valid.size();
    msj_dictionary_result lay;
    std::vector<int32_t> codes(rows, 0x77777777);
    dcm_dictionary(c.offsets.data(), c.valid.data(), rows, n_rows, c.bytes.data(), bytes_len, codes.data(), nullptr, nullptr, 0, nullptr, 0, flags,
                   order, &lay);
    const uint64_t R = n_rows ? *n_rows : rows;
    CHECK(lay.n_rows == R && lay.flags == flags);
    if (R > rows) {
        CHECK(lay.code == MSJ_CAPACITY && lay.n_values == 0 && lay.n_distinct == 0);
        for (int32_t x : codes) CHECK(x == 0x77777777);
        return codes;
    }
    CHECK(lay.code == 0 && lay.n_distinct <= lay.n_values && lay.n_values <= R);
    if (form == 3) return codes;
    uint64_t cap = lay.n_distinct, room = lay.dict_bytes;
    if (form == 1 && cap) cap--;
    if (form == 2 && room) room--;
    if (form == 4) cap = 0, room = 0;
    std::vector<uint64_t> d_off(cap + 1, 0x7777777777777777ull);
    std::vector<uint32_t> d_first(cap, 0x77777777u);
    std::vector<uint8_t> d_bytes(room, kFill);
    std::vector<int32_t> again(rows, 0x77777777);
    msj_dictionary_result res;
    dcm_dictionary(c.offsets.data(), c.valid.data(), rows, n_rows, c.bytes.data(), bytes_len, again.data(), d_off.data(), d_first.data(), cap,
                   d_bytes.data(), room, flags, order, &res);
    const bool clipped = cap < lay.n_distinct || room < lay.dict_bytes;
    CHECK(res.code == (clipped ? MSJ_CAPACITY : 0) && res.n_distinct == lay.n_distinct && res.dict_bytes == lay.dict_bytes);
    CHECK(res.n_values == lay.n_values && again == codes && d_off[0] == 0);
    uint64_t values = 0;
    for (uint64_t k = 0; k < rows; k++) {
        if (k >= R) {
            CHECK(again[k] == 0x77777777);
            continue;
        }
        const msj::dict::Row y = msj::dict::row_of(c.offsets.data(), c.valid.data(), k, bytes_len);
        CHECK((again[k] == -1) == !y.has);
        if (!y.has) continue;
        values++;
        CHECK(again[k] >= 0 && (uint64_t)again[k] < res.n_distinct);
        if ((uint64_t)again[k] >= cap) continue;
        const uint32_t f = d_first[again[k]];
        CHECK(f <= k && again[f] == again[k]);
        const msj::dict::Row z = msj::dict::row_of(c.offsets.data(), c.valid.data(), f, bytes_len);
        CHECK(z.has && z.len == y.len && memcmp(c.bytes.data() + z.at, c.bytes.data() + y.at, y.len) == 0);
        CHECK(d_off[again[k] + 1] - d_off[again[k]] == y.len);
        for (uint64_t b = 0; b < y.len && d_off[again[k]] + b < room; b++) CHECK(d_bytes[d_off[again[k]] + b] == c.bytes[y.at + b]);
    }
    CHECK(values == res.n_values);
    for (uint64_t e = 1; e < cap; e++) CHECK(d_first[e - 1] < d_first[e] && d_off[e] <= d_off[e + 1]);
    if (cap == res.n_distinct) CHECK(d_off[cap] == res.dict_bytes);
    return codes;
}

void all_forms(const Column &c, uint64_t bytes_len, const uint64_t *n_rows) {
    const std::vector<int32_t> want = run(c, bytes_len, n_rows, 0, 0, 0);
    for (uint32_t flags = 0; flags < 2; flags++)
        for (int order = 0; order < 2; order++)
            for (int form = 0; form < 5; form++) CHECK(run(c, bytes_len, n_rows, flags, order, form) == want);
}

Column pinned() {
    Column c;
    c.offsets.push_back(0);
    const std::string big(3000, 'z');
    const std::string values[] = {"red", "green", "", "red", "re", "redd", big, "blue", "", big, big.substr(0, 2999) + "y", "green"};
    for (int round = 0; round < 3; round++)
        for (const std::string &v : values) {
            c.bytes.insert(c.bytes.end(), v.begin(), v.end());
            c.offsets.push_back(c.bytes.size());
            c.valid.push_back(1);
            if (round == 1) c.offsets.push_back(c.bytes.size()), c.valid.push_back(0);  // a null row behind each
        }
    return c;
}

}  // namespace

int main() {
    const Column pin = pinned();
    const uint64_t rows = pin.valid.size(), len = pin.bytes.size();
    all_forms(pin, len, nullptr);
    for (uint64_t r : std::vector<uint64_t>{0, 1, rows - 1, rows, rows + 1, ~(uint64_t)0}) all_forms(pin, len, &r);
    all_forms(Column{{0}, {}, {}}, 0, nullptr);
    for (int round = 0; round < 300; round++) {
        Column c = pin;
        const int hits = 1 + (int)(rnd() % 6);
        for (int j = 0; j < hits; j++) {
            const uint64_t k = rnd() % c.offsets.size();
            switch (rnd() % 5) {
                case 0: c.offsets[k] = rnd() % (len + 3); break;
                case 1: c.offsets[k] = rnd(); break;
                case 2: c.offsets[k] = len + 1 + rnd() % 5; break;
                case 3: c.valid[rnd() % rows] = (uint8_t)rnd(); break;
                default: c.offsets[k] = k ? c.offsets[k - 1] - (k > 1 && c.offsets[k - 1] ? 1 : 0) : 0; break;
            }
        }
        uint64_t short_len = len;
        if (round % 3 == 0) {  // a window of bytes shorter than the offsets say, at its exact size
            short_len = rnd() % (len + 1);
            c.bytes.resize(short_len);
            c.bytes.shrink_to_fit();
        }
        all_forms(c, short_len, nullptr);
        if (round % 7 == 0) {
            const uint64_t r = rnd() % (rows + 2);
            all_forms(c, short_len, &r);
        }
    }
    if (failures) return 1;
    printf("dictionary_sanitize ok\n");
    return 0;
}
