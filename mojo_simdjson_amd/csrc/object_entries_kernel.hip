// An object's members as a map column -- msj_object_entries_device (include/msj_stage1.h): msj_array_elements_device with
// objects as the rows and two records per entry, the key's and the value's, so that an object whose keys are data
// ("attrs":{"color":"red","size":"L"}, a map of maps) is a column too.  The arithmetic that is new -- the row test with '{',
// the candidate test, the entry test -- is object_entries_math.h, host + device and checked on the CPU by
// tests/test_object_entries_math.py; everything else is array_elements_math.h's and select_math.h's.  R =
// d_rows_select->n_documents is read on the device by every kernel: the host never learns it.
//
// As in array_elements_kernel.hip there is no walk and no counter per row: an entry's place in the output is the number of
// key tokens of entries in front of it in the window, a row's offset that number just behind the row's own token.  The
// kernels and their eight launches are rows_block.h's; this file holds the policy that makes them this call
// (msj_oent::Entries) and the entry points.  The launches, all on the caller's stream, behind a 64-byte memset of the call's
// state:
//   rows_live, rows_ranks, rows_place<'{'>, rows_order   the kernels over rows with '{' as the container
//   items_count<Entries>   a block of 1 024 tokens, 4 per lane; the type word as one 4-byte load, the depths as one 16-byte
//              load, one token of halo BEHIND the block (type[base + 1 024], 0 at or past n): a lane takes its successor's
//              first type byte from LDS.  A candidate is a '"' with ':' behind it; it finds its row among the staged ones by
//              binary search and tests itself against that row's descriptor, one 16-byte gather.  Ends early: a block without
//              a candidate, a block no row reaches, a block inside ONE row whose partner lies in front of it
//   items_scan<Entries>    one workgroup of 1 024: the exclusive sum over the blocks' counts, then the result, d_offsets[R] and
//              the two select results
//   items_emit<Entries>    the same block shape.  An entry's position is the block's prefix + the exclusive sum inside the
//              block; the key's record (token i) and the value's (token i + 2, gathered: it may lie in the next block) leave
//              as one 16-byte store each when the position is below entries_capacity.  A staged row that starts in the block
//              marks its token in LDS; the lane that holds the token writes the dense row's offset
//   rows_finish   d_offsets[r] and d_valid[r] from the row's word
// Safety: a row's token is used only when it is below n; every index from d_match is checked before it is used; an entry has
// i + 2 < m < n, so tokens i + 1 and i + 2 index the arrays; the type behind a token is read only below n; every store to
// d_keys / d_values is checked against entries_capacity.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/msj_stage1.h"
#include "launch.h"
#include "object_entries_math.h"
#include "rows_block.h"

namespace msj_oent {

using namespace msj_rows;
namespace oent = msj::oent;

static_assert(sizeof(msj_object_entries_result) == 48, "ABI");

// rows_block.h's policy: the rows are objects, an item is an entry -- its key token --, two records each
struct Entries {
    static constexpr uint32_t kContainer = oent::kContainer;
    struct Out {
        msj_field *keys, *values;  // (keys and values come together: the entry point checks)
        uint64_t capacity;
        msj_object_entries_result *result;
        msj_select_documents_result *keys_select, *values_select;
        __device__ bool have() const { return keys != nullptr; }
        __device__ msj_select_documents_result *no_bits_select() const { return values_select; }  // (a key is a string)
    };
    // a candidate is a '"' with ':' behind it: the halo is the token behind the block, 0 at or past n; a lane takes its
    // successor's first type byte from LDS
    static __device__ __forceinline__ Lane load_lane(uint64_t n, uint64_t base, const uint8_t *__restrict__ type, const int32_t *__restrict__ depth,
                                                     uint32_t *s_type) {
        Lane l;
        const uint64_t mine = base + (uint64_t)threadIdx.x * kPer;
        l.t = load_token_quad(type, depth, mine, n);  // (tokens at or past n read as type 0)
        s_type[threadIdx.x] = l.t.tw;
        uint32_t halo = 0;
        if (threadIdx.x == kThreads - 1 && base + kBlock < n) halo = type[base + kBlock];
        __syncthreads();
        const uint32_t behind = threadIdx.x + 1 < kThreads ? s_type[threadIdx.x + 1] & 0xFFu : halo;
        l.cand = 0;
#pragma unroll
        for (int k = 0; k < kPer; k++) {
            const uint32_t t = (l.t.tw >> (8 * k)) & 0xFFu;
            const uint32_t t_next = k + 1 < kPer ? (l.t.tw >> (8 * (k + 1))) & 0xFFu : behind;
            if (mine + k < n && oent::is_key_candidate(t, t_next)) l.cand |= 1u << k;
        }
        return l;
    }
    static __device__ __forceinline__ bool is_item(uint64_t i, int32_t depth_i, const Desc &d) { return oent::is_entry_of(i, depth_i, d); }
    // the key's record (token i) and the value's (token i + 2, gathered: it may lie in the next block).  (An entry: i + 2 < m < n)
    static __device__ __forceinline__ uint32_t store(const Out &o, uint64_t pos, uint64_t i, const ItemValues &values) {
        store_field(o.keys, pos, values.field(i));
        const msj_field v = values.field(i + 2);
        store_field(o.values, pos, v);
        return (v.flags & kFieldNoBits) != 0;
    }
    static __device__ __forceinline__ void results(const Out &o, const ItemTotals &t) {
        msj_object_entries_result r;
        r.code = t.stop_code ? t.stop_code : oent::entries_code(t.n_items, o.have(), o.capacity);
        r.flags = 0;
        r.n_rows = t.n_rows;
        r.n_objects = t.n_containers;
        r.n_entries = t.n_items;
        r.n_other = t.n_other;
        r.n_no_bits = 0;  // (items_emit's)
        *o.result = r;
        if (o.keys_select) *o.keys_select = items_select(r.code, t.n_items);
        if (o.values_select) *o.values_select = items_select(r.code, t.n_items);
    }
};

}  // namespace msj_oent

extern "C" uint64_t msj_object_entries_workspace_bytes(uint64_t n, uint64_t capacity) { return msj_rows::work_bytes(n, capacity); }

extern "C" int msj_launch_object_entries(const msj_token_view &t, const msj_number_view &nv, const msj_field *d_rows,
                                         const msj_select_documents_result *d_rows_select, uint64_t *d_offsets, uint8_t *d_valid,
                                         uint64_t capacity, msj_field *d_keys, msj_field *d_values, uint64_t entries_capacity,
                                         msj_object_entries_result *d_result, msj_select_documents_result *d_keys_select,
                                         msj_select_documents_result *d_values_select, void *d_ws, void *stream) {
    using msj_oent::Entries;
    return msj_rows::launch_items<Entries>(t, nv, d_rows, d_rows_select, d_offsets, d_valid, capacity,
                                           Entries::Out{d_keys, d_values, entries_capacity, d_result, d_keys_select, d_values_select}, d_ws, stream);
}
