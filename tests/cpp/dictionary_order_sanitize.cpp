// Stand-alone program (its own main; built by tests/test_dictionary_order_sanitizers.py with -fsanitize=address,undefined): the
// host form of the arithmetic of msj_dictionary_order_device and msj_rank_rows_device (tests/dictionary_order_math_host.cpp
// over csrc/dictionary_order_math.h) on arrays from anywhere.  The word fetch -- the one reader of a dictionary's bytes,
// shared with the kernels -- at every start phase, every value end at the capacity minus 0 .. 8 and every misalignment of the
// base, the bytes ending exactly where their allocation ends and, through a byte source that checks every index, never
// starting in front of it; a pinned corpus; and then, round after round, hostile arrays: offsets from anywhere, V below, at
// and above the room, both paths, budgets of 1 .. 3 and 64 rounds, CONTINUE over state from anywhere, codes from anywhere.
// Every array is a std::vector of exactly its size, so a read or a write outside is the sanitizer's to report.  Asserted
// here, by a comparator that shares nothing with the header (memcmp, then length): the order and the ranks of every complete
// call; that every entry written lies below V and nothing at or past V is written.  NOT part of the product.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../dictionary_order_math_host.cpp"

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

constexpr uint32_t kFill = 0xA5A5A5A5u;
const uint8_t kAlphabet[6] = {0x00, 'a', 'b', 0x7f, 0x80, 0xff};

// a byte source that refuses what the definition forbids: a byte outside [0, capacity), a word that is not aligned or not
// wholly inside
struct CheckedBytes {
    const uint8_t *p;
    uint64_t capacity;
    uint64_t misalign() const { return (uint64_t)(reinterpret_cast<uintptr_t>(p) & 7u); }
    uint8_t byte(uint64_t i) const {
        CHECK(i < capacity);
        return p[i];
    }
    uint64_t word(uint64_t i) const {
        CHECK(i + 8 <= capacity && i + 8 >= 8 && ((reinterpret_cast<uintptr_t>(p) + i) & 7u) == 0);
        uint64_t w;
        memcpy(&w, p + i, 8);
        return w;
    }
};

void fetch_everywhere() {
    for (uint64_t mis = 0; mis < 8; mis++)
        for (uint64_t cap = 0; cap < 40; cap++) {
            std::vector<uint8_t> room(mis + cap);  // (the allocation is 8-aligned: the bytes start `mis` off and end at its end)
            for (auto &b : room) b = (uint8_t)rnd();
            const uint8_t *bytes = room.data() + mis;
            for (uint64_t back = 0; back <= 8 && back <= cap; back++)
                for (uint64_t begin = 0; begin <= cap - back; begin++)
                    for (uint64_t depth = 0; depth <= 16; depth += 8) {
                        const uint64_t len = cap - back - begin;
                        const Word got = fetch_word(MemoryBytes{bytes}, cap, begin, len, depth);
                        const Word same = fetch_word(CheckedBytes{bytes, cap}, cap, begin, len, depth);
                        uint64_t want = 0, n = len > depth ? std::min<uint64_t>(8, len - depth) : 0;
                        for (uint64_t k = 0; k < n; k++) want |= (uint64_t)bytes[begin + depth + k] << (8 * (7 - k));
                        CHECK(got.word == want && got.nvalid == n && same.word == want && same.nvalid == n);
                    }
        }
}

struct Made {
    std::vector<uint64_t> offsets;
    std::vector<uint8_t> bytes;
};
// the values back to back; an entry without a value is made by the caller
Made layout(const std::vector<std::string> &values) {
    Made m;
    m.offsets.push_back(0);
    for (const auto &v : values) {
        m.bytes.insert(m.bytes.end(), v.begin(), v.end());
        m.offsets.push_back(m.bytes.size());
    }
    return m;
}
bool has_value(const Made &m, uint64_t c) { return m.offsets[c] <= m.offsets[c + 1] && m.offsets[c + 1] <= m.bytes.size(); }
int compare(const Made &m, uint32_t a, uint32_t b) {  // memcmp, then length
    const uint64_t la = m.offsets[a + 1] - m.offsets[a], lb = m.offsets[b + 1] - m.offsets[b];
    const int c = std::min(la, lb) ? memcmp(m.bytes.data() + m.offsets[a], m.bytes.data() + m.offsets[b], std::min(la, lb)) : 0;
    return c ? c : la < lb ? -1 : la > lb ? 1 : 0;
}

void check_complete(const Made &m, uint64_t V, const std::vector<uint32_t> &sorted, const std::vector<uint32_t> &rank,
                    const msj_dictionary_order_result &res) {
    std::vector<uint32_t> want;
    for (uint32_t c = 0; c < V; c++)
        if (has_value(m, c)) want.push_back(c);
    const uint64_t n_values = want.size();
    std::stable_sort(want.begin(), want.end(), [&](uint32_t a, uint32_t b) { return compare(m, a, b) < 0; });
    for (uint32_t c = 0; c < V; c++)
        if (!has_value(m, c)) want.push_back(c);
    CHECK(res.n_values == n_values && res.n_tied == 0 && res.code == 0);
    uint64_t equal = 0;
    for (uint64_t p = 0; p < V; p++) {
        CHECK(sorted[p] == want[p]);
        if (p >= n_values) {
            CHECK(rank[want[p]] == MSJ_ORDER_NO_RANK);
            continue;
        }
        uint64_t first = p;
        while (first > 0 && compare(m, want[first - 1], want[p]) == 0) first--;
        CHECK(rank[want[p]] == first);
        equal += first != p;
    }
    CHECK(res.n_equal == equal);
}

// one order by chains of `budget` rounds, the paths taking turns
void order_of(const Made &m, uint64_t V, uint64_t capacity, uint32_t budget, bool valid_layout) {
    std::vector<uint32_t> sorted(capacity, kFill), rank(capacity, kFill);
    std::vector<uint64_t> offsets(m.offsets.begin(), m.offsets.begin() + std::min<uint64_t>(m.offsets.size(), capacity + 1));
    offsets.resize(capacity + 1, 0);
    msj_dictionary_order_result res;
    uint64_t depth = 0;
    for (uint32_t call = 0;; call++) {
        const int32_t rc = dom_dictionary_order(1, offsets.data(), m.bytes.empty() ? nullptr : m.bytes.data(), m.bytes.size(), V, nullptr, capacity, depth,
                                                budget, call ? MSJ_ORDER_CONTINUE : 0, 1 + (call & 1), capacity ? sorted.data() : nullptr,
                                                capacity ? rank.data() : nullptr, &res, nullptr);
        CHECK(rc == 0);
        if (rc != 0) return;
        if (V > capacity) {
            CHECK(res.code == MSJ_CAPACITY && res.n_entries == V && res.depth == 0 && res.n_tied == 0);
            for (uint64_t p = 0; p < capacity; p++) CHECK(sorted[p] == kFill && rank[p] == kFill);
            return;
        }
        for (uint64_t p = 0; p < capacity; p++) CHECK(p < V ? sorted[p] < V && (rank[p] < V || rank[p] == MSJ_ORDER_NO_RANK) : sorted[p] == kFill && rank[p] == kFill);
        if (res.code == 0) break;
        CHECK(res.code == MSJ_CAPACITY && res.n_tied > 0 && res.depth == depth + 8ull * budget);
        depth = res.depth;
        if (call > 4000) {
            CHECK(!"the chain ends");
            return;
        }
    }
    if (valid_layout) check_complete(m, V, sorted, rank, res);
}

std::string word(uint64_t n) {
    std::string s;
    for (uint64_t k = 0; k < n; k++) s.push_back((char)kAlphabet[rnd() % 6]);
    return s;
}

void pinned() {
    const std::vector<std::string> nul = {std::string("a\0", 2), "a", std::string("a\0\0", 3), "", std::string("\0", 1), "aaaaaaaa", std::string("aaaaaaaa\0", 9), "aaaaaaa"};
    const std::vector<std::string> sign = {"\x80", "\x7f", "\xff", "a", "\xff\x01", "\x7f\xff"};
    const std::vector<std::string> equal = {"bbbbbbbbbbbbbbbb", "aaaaaaaa", "bbbbbbbbbbbbbbbb", "aaaaaaaa", "", ""};
    for (const auto *v : {&nul, &sign, &equal})
        for (uint32_t budget : {1u, 2u, 3u, 64u}) {
            const Made m = layout(*v);
            order_of(m, v->size(), v->size(), budget, true);
            order_of(m, v->size(), v->size() + 3, budget, true);
            order_of(m, v->size(), v->size() - 1, budget, true);
        }
    order_of(layout({}), 0, 0, 1, true);
    order_of(layout({}), 0, 4, 1, true);
}

void hostile(uint32_t round) {
    const uint64_t V = rnd() % 40;
    std::vector<std::string> values;
    const std::string shared = word((const uint64_t[]){0, 3, 8, 9, 16, 24}[rnd() % 6]);
    for (uint64_t c = 0; c < V; c++) values.push_back((rnd() % 5 ? shared : std::string()) + word(rnd() % 12));
    Made m = layout(values);
    const uint32_t budget = (const uint32_t[]){1, 2, 3, 64}[rnd() % 4];
    if (round % 3 == 0) {  // a real dictionary, duplicates and all
        order_of(m, V, V + rnd() % 3, budget, true);
        return;
    }
    // offsets from anywhere
    for (auto &o : m.offsets)
        if (rnd() % 4 == 0) o = (const uint64_t[]){0, m.bytes.size(), m.bytes.size() + 1, rnd() % (m.bytes.size() + 2), ~0ull, rnd()}[rnd() % 6];
    const uint64_t capacity = V + rnd() % 3 - (V && rnd() % 8 == 0);
    if (round % 3 == 1) {
        order_of(m, V, capacity, budget, false);
        return;
    }
    // CONTINUE over state from anywhere; codes from anywhere through the ranks it leaves
    if (V > capacity || capacity == 0) return;
    std::vector<uint32_t> sorted(capacity), rank(capacity);
    for (auto &x : sorted) x = rnd() % 3 ? (uint32_t)(rnd() % (V + 2)) : (uint32_t)rnd();
    for (auto &x : rank) x = rnd() % 3 ? (uint32_t)(rnd() % (V + 2)) : rnd() % 2 ? (uint32_t)rnd() : MSJ_ORDER_NO_RANK;
    std::vector<uint64_t> offsets(m.offsets);
    offsets.resize(capacity + 1, 0);
    msj_dictionary_order_result res;
    const int32_t rc = dom_dictionary_order(1, offsets.data(), m.bytes.empty() ? nullptr : m.bytes.data(), m.bytes.size(), V, nullptr, capacity,
                                            8 * (rnd() % 4), budget, MSJ_ORDER_CONTINUE, 1 + rnd() % 2, sorted.data(), rank.data(), &res, nullptr);
    CHECK(rc == 0 && res.n_entries == V);
    const uint64_t R = rnd() % 50;
    std::vector<int32_t> codes(R);
    for (auto &c : codes) c = rnd() % 3 ? (int32_t)(rnd() % (V + 3)) - 2 : (int32_t)rnd();
    std::vector<msj_field> fields(R);
    if (R) memset(fields.data(), 0xA5, R * sizeof(msj_field));
    msj_rank_rows_result rres;
    msj_select_documents_result sel;
    res.code = 0;
    const int32_t rc2 = dom_rank_rows(1, R ? codes.data() : nullptr, R, nullptr, rank.data(), capacity, &res, R ? fields.data() : nullptr, R, &rres, &sel);
    CHECK(rc2 == 0 && rres.code == 0 && rres.n_ranked + rres.n_null + rres.n_unknown == R && sel.n_found == rres.n_ranked);
    for (uint64_t k = 0; k < R; k++) {
        const bool ranked = codes[k] >= 0 && (uint64_t)codes[k] < V && rank[codes[k]] != MSJ_ORDER_NO_RANK;
        CHECK(fields[k].token == 0xFFFFFFFFu && fields[k].code == (ranked ? 0 : 20) && fields[k].type == (ranked ? 'l' : 0));
        if (ranked) CHECK(fields[k].bits == rank[codes[k]]);
    }
}

}  // namespace

int main() {
    fetch_everywhere();
    pinned();
    for (uint32_t round = 0; round < 4000; round++) hostile(round);
    if (failures) {
        printf("dictionary_order_sanitize: %d failures\n", failures);
        return 1;
    }
    printf("dictionary_order_sanitize ok\n");
    return 0;
}
