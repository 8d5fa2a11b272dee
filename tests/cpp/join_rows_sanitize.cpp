// Stand-alone program (its own main; built by tests/test_join_rows_sanitizers.py with -fsanitize=address,undefined): the host
// form of the arithmetic of msj_join_rows_device (tests/join_rows_math_host.cpp over csrc/join_rows_math.h) on arrays from
// anywhere.  A pinned corpus -- the four kinds of one small join, keys at the edges of [0, G), all-null sides, every key
// equal -- and then, round after round, hostile key columns: wild keys (-2, -1, G, INT32_MIN, INT32_MAX, random words),
// counts on the "device" below, at and above the rooms, a G above keys_capacity, pair rooms around M.  Every array is a
// std::vector of exactly its size, so a read or a write outside is the sanitizer's to report, and every shift and signed
// operation of the header is the undefined-behaviour sanitizer's.  Asserted here, by loops that share nothing with the
// header's search: the pinned pairs; that the pairs are those of the double loop over (l, r) in order; that the offsets
// count them; that nothing at or past M, the room or offsets[L] is written.  NOT part of the product.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "../join_rows_math_host.cpp"

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
constexpr uint64_t kFill64 = 0xA5A5A5A5A5A5A5A5ull;
using Pairs = std::vector<std::pair<uint32_t, uint32_t>>;

// the definition as a double loop
Pairs definition(const std::vector<int32_t> &lk, uint64_t L, const std::vector<int32_t> &rk, uint64_t R, uint64_t G, uint32_t kind,
                 std::vector<uint64_t> *offsets) {
    Pairs out;
    offsets->assign(1, 0);
    for (uint64_t l = 0; l < L; l++) {
        uint64_t c = 0;
        const bool has_key = lk[l] >= 0 && (uint64_t)lk[l] < G;
        for (uint64_t r = 0; has_key && r < R; r++) {
            if (rk[r] != lk[l]) continue;
            if (kind == MSJ_JOIN_INNER || kind == MSJ_JOIN_LEFT || (kind == MSJ_JOIN_SEMI && c == 0)) out.push_back({(uint32_t)l, (uint32_t)r});
            c++;
        }
        if (c == 0 && (kind == MSJ_JOIN_LEFT || kind == MSJ_JOIN_ANTI)) out.push_back({(uint32_t)l, MSJ_JOIN_NO_ROW});
        offsets->push_back(out.size());
    }
    return out;
}

Pairs join_of(const std::vector<int32_t> &lk, const std::vector<int32_t> &rk, uint64_t G, uint32_t kind) {
    std::vector<uint64_t> want_off, off(lk.size() + 1, kFill64);
    const Pairs want = definition(lk, lk.size(), rk, rk.size(), G, kind, &want_off);
    std::vector<uint32_t> a(want.size(), kFill), b(want.size(), kFill);
    msj_join_rows_result res;
    CHECK(jrm_join_rows(1, lk.data(), lk.size(), nullptr, rk.data(), rk.size(), nullptr, G, nullptr, G, kind, a.data(), b.data(), a.size(), off.data(), &res,
                        nullptr, nullptr) == 0);
    CHECK(res.code == 0 && res.n_pairs == want.size() && off == want_off);
    Pairs got;
    for (size_t j = 0; j < a.size(); j++) got.push_back({a[j], b[j]});
    CHECK(got == want);
    return got;
}

void pinned() {
    const uint32_t N = MSJ_JOIN_NO_ROW;
    const std::vector<int32_t> lk = {1, -1, 0, 1, 4}, rk = {1, 0, 1, -2, 3};
    CHECK(join_of(lk, rk, 5, MSJ_JOIN_INNER) == (Pairs{{0, 0}, {0, 2}, {2, 1}, {3, 0}, {3, 2}}));
    CHECK(join_of(lk, rk, 5, MSJ_JOIN_LEFT) == (Pairs{{0, 0}, {0, 2}, {1, N}, {2, 1}, {3, 0}, {3, 2}, {4, N}}));
    CHECK(join_of(lk, rk, 5, MSJ_JOIN_SEMI) == (Pairs{{0, 0}, {2, 1}, {3, 0}}));
    CHECK(join_of(lk, rk, 5, MSJ_JOIN_ANTI) == (Pairs{{1, N}, {4, N}}));
    CHECK(join_of(lk, rk, 1, MSJ_JOIN_INNER) == (Pairs{{2, 1}}));  // (G = 1: only code 0 is a key)
    CHECK(join_of(lk, rk, 0, MSJ_JOIN_LEFT).size() == 5 && join_of(lk, rk, 0, MSJ_JOIN_INNER).empty());
    const std::vector<int32_t> edges = {INT32_MIN, INT32_MAX, -1, -2, 299, 300, 0};
    CHECK(join_of(edges, edges, 300, MSJ_JOIN_INNER) == (Pairs{{4, 4}, {6, 6}}));
    CHECK(join_of(std::vector<int32_t>(7, 2), std::vector<int32_t>(9, 2), 3, MSJ_JOIN_INNER).size() == 63);
    CHECK(join_of(std::vector<int32_t>(7, -1), std::vector<int32_t>(9, -1), 3, MSJ_JOIN_ANTI).size() == 7);
    CHECK(join_of({}, rk, 5, MSJ_JOIN_LEFT).empty() && join_of(lk, {}, 5, MSJ_JOIN_LEFT).size() == 5);
    CHECK(key_digits(256) == 1 && key_digits(257) == 2 && key_digits(65537) == 3 && key_digits((1u << 24) + 1) == 4 && key_digits(1ull << 40) == 4);
}

int32_t hostile_key(uint64_t G) {
    switch (rnd() % 10) {
        case 0: return -1;
        case 1: return -2;
        case 2: return (int32_t)G;
        case 3: return rnd() % 2 ? INT32_MIN : INT32_MAX;
        case 4: return (int32_t)(uint32_t)rnd();
        case 5: return (int32_t)(rnd() % 3);  // a hot key
        default: return (int32_t)(rnd() % (G + 1));
    }
}

void hostile_round() {
    static const uint64_t gs[] = {0, 1, 2, 5, 255, 256, 257, 1000, 65536, 65537, 70000};
    const uint64_t G = gs[rnd() % 11], keys_capacity = rnd() % 8 == 0 && G ? G - 1 : G + rnd() % 3;
    const uint64_t left_rows = rnd() % 70, right_rows = rnd() % 70;
    const uint64_t L = rnd() % 8 == 0 ? left_rows + 1 + rnd() % 3 : rnd() % (left_rows + 1);
    const uint64_t R = rnd() % 8 == 0 ? right_rows + 1 + rnd() % 3 : rnd() % (right_rows + 1);
    const uint32_t kind = (uint32_t)(rnd() % 4);
    std::vector<int32_t> lk(left_rows), rk(right_rows);
    for (int32_t &k : lk) k = hostile_key(G);
    for (int32_t &k : rk) k = hostile_key(G);
    const bool over = L > left_rows || R > right_rows || G > keys_capacity;
    std::vector<uint64_t> want_off;
    Pairs want;
    if (!over) want = definition(lk, L, rk, R, G, kind, &want_off);
    const uint64_t M = want.size();
    const uint64_t room = rnd() % 4 == 0 ? (M ? M - 1 : 0) : rnd() % 4 == 1 ? rnd() % (M + 1) : M + rnd() % 3;
    const bool with_right = rnd() % 4 != 0, with_off = rnd() % 4 != 0, counts_given = rnd() % 2;
    std::vector<uint32_t> a(room, kFill), b(with_right ? room : 0, kFill);
    std::vector<uint64_t> off(with_off ? left_rows + 1 : 0, kFill64), n(3);
    n[0] = L, n[1] = R, n[2] = G;
    // (a count not given on the "device" is the room: then L == left_rows)
    const uint64_t lr = counts_given ? left_rows : L, rr = counts_given ? right_rows : R;
    if (!counts_given && over && (L > left_rows || R > right_rows)) return;  // (rows beyond the vectors cannot be passed as rooms)
    msj_join_rows_result res;
    msj_select_documents_result ls, rs;
    if (!counts_given) lk.resize(lr), rk.resize(rr);
    if (!counts_given && with_off) off.assign(lr + 1, kFill64);
    CHECK(jrm_join_rows(1, lr ? lk.data() : nullptr, lr, counts_given ? &n[0] : nullptr, rr ? rk.data() : nullptr, rr, counts_given ? &n[1] : nullptr,
                        counts_given ? 12345 : G, counts_given ? &n[2] : nullptr, keys_capacity, kind, room ? a.data() : nullptr,
                        with_right && room ? b.data() : nullptr, room, with_off ? off.data() : nullptr, &res, &ls, &rs) == 0);
    CHECK(res.flags == kind && res.n_left == L && res.n_right == R && res.n_keys == G);
    CHECK(ls.code == res.code && rs.code == res.code && ls.n_documents == res.n_pairs && rs.n_found == res.n_pairs && ls.n_paths == 1);
    if (over) {
        CHECK(res.code == MSJ_CAPACITY && res.n_pairs + res.n_left_matched + res.n_left_null + res.n_right_null == 0);
        for (uint32_t x : a) CHECK(x == kFill);
        for (uint32_t x : b) CHECK(x == kFill);
        for (uint64_t x : off) CHECK(x == kFill64);
        return;
    }
    CHECK(res.n_pairs == M && res.code == (M > room ? MSJ_CAPACITY : 0));
    uint64_t l_null = 0, r_null = 0;
    for (uint64_t l = 0; l < L; l++) l_null += !(lk[l] >= 0 && (uint64_t)lk[l] < G);
    for (uint64_t r = 0; r < R; r++) r_null += !(rk[r] >= 0 && (uint64_t)rk[r] < G);
    CHECK(res.n_left_null == l_null && res.n_right_null == r_null && res.n_left_matched <= L - l_null);
    if (with_off) {
        for (uint64_t l = 0; l <= L; l++) CHECK(off[l] == want_off[l]);
        for (uint64_t l = L + 1; l < off.size(); l++) CHECK(off[l] == kFill64);
    }
    const uint64_t written = M > room ? 0 : M;
    for (uint64_t j = 0; j < written; j++) CHECK(a[j] == want[j].first && (!with_right || b[j] == want[j].second));
    for (uint64_t j = written; j < room; j++) CHECK(a[j] == kFill && (!with_right || b[j] == kFill));
}

}  // namespace

int main() {
    pinned();
    for (uint32_t round = 0; round < 4000; round++) hostile_round();
    if (failures) return printf("%d checks failed\n", failures), 1;
    printf("join_rows_sanitize ok\n");
    return 0;
}
