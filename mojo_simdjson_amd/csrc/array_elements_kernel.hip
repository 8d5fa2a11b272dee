// The arrays inside list rows as a list column -- msj_array_elements_device (include/msj_stage1.h): msj_array_column_device
// with ANY ascending msj_field records as the rows, so that a list of lists ("coordinates":[[x,y],...]) and a list inside a
// list of structs (items[*].tags) are list columns too, and the call runs on its own output to any depth.  The arithmetic
// that is new -- the verdict on the rows, the live rows, the word a row keeps, a row's offset -- is array_elements_math.h,
// host + device and checked on the CPU by tests/test_array_elements_math.py; the candidate and element tests and the
// descriptor are array_column_math.h's, the row search and the order test select_elements_math.h's, an element's record
// select_math.h's value_field.  R = d_rows_select->n_documents is read on the device by every kernel: the host never learns it.
//
// No walk and no counter per row: the live rows (records with code 0) ascend and each token belongs to one of them, so an
// element's place in the output is the number of element tokens in front of it in the window, and a row's offset is that
// number just behind the row's own token.  The kernels and their eight launches are rows_block.h's, shared with
// object_entries_kernel.hip; this file holds the policy that makes them this call (msj_aelem::Elements) and the entry
// points.  The launches, all on the caller's stream, behind a 64-byte memset of the call's state:
//   rows_live, rows_ranks, rows_place<'['>, rows_order   the kernels over rows with '[' as the container: the live rows
//              counted and ranked, start[j] and the 16-byte descriptor per dense row, the word {j, live} per row, n_arrays /
//              n_other; a violation of the order sets the state's flag, and every later kernel returns at once when it is set
//   items_count<Elements>   a block of 1 024 tokens, 4 per lane; the type word as one 4-byte load, the depths as one 16-byte
//              load, one token of halo in FRONT of the block.  Two searches in start[] give the rows that can own a token of
//              the block or start in it -- at most 1 025 --, staged in LDS; a candidate (behind '[' or ',', no closer) finds
//              its row there by binary search and tests itself against that row's descriptor, one 16-byte gather.  Ends
//              early: a block without a candidate, a block no row reaches, a block inside ONE row whose partner lies in
//              front of it
//   items_scan<Elements>    one workgroup of 1 024: the exclusive sum over the blocks' counts, then the result, d_offsets[R]
//              and d_elements_select
//   items_emit<Elements>    the same block shape.  An element's position is the block's prefix + the exclusive sum inside the
//              block; its record leaves as one 16-byte store when the position is below elements_capacity.  A staged row
//              that starts in the block marks its token in LDS; the lane that holds the token writes the dense row's offset,
//              also in a block that holds no element
//   rows_finish   d_offsets[r] and d_valid[r] from the row's word.  Last, so that an order violation leaves both untouched
// Safety: a row's token is used only when it is below n; every index from d_match is checked before it is used; dense numbers
// are below min(live rows, n, capacity); rows are below R <= capacity; every store to d_elements is checked against
// elements_capacity.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/msj_stage1.h"
#include "array_elements_math.h"
#include "launch.h"
#include "rows_block.h"

namespace msj_aelem {

using namespace msj_rows;

static_assert(sizeof(msj_array_column_result) == 48, "ABI");

// rows_block.h's policy: the rows are arrays, an item is an element, one record each
struct Elements {
    static constexpr uint32_t kContainer = '[';
    struct Out {
        msj_field *elements;
        uint64_t capacity;
        msj_array_column_result *result;
        msj_select_documents_result *elements_select;
        __device__ bool have() const { return elements != nullptr; }
        __device__ msj_select_documents_result *no_bits_select() const { return elements_select; }
    };
    // a candidate stands behind '[' or ',': the halo is the token in front of the block
    static __device__ __forceinline__ Lane load_lane(uint64_t n, uint64_t base, const uint8_t *__restrict__ type, const int32_t *__restrict__ depth,
                                                     uint32_t *s_type) {
        return load_lane_front(n, base, type, depth, s_type, [n](uint64_t i) { return i < n; });
    }
    static __device__ __forceinline__ bool is_item(uint64_t i, int32_t depth_i, const Desc &d) { return is_element_of(i, depth_i, d); }
    static __device__ __forceinline__ uint32_t store(const Out &o, uint64_t pos, uint64_t i, const ItemValues &values) {
        const msj_field r = values.field(i);
        store_field(o.elements, pos, r);
        return (r.flags & kFieldNoBits) != 0;
    }
    static __device__ __forceinline__ void results(const Out &o, const ItemTotals &t) {
        msj_array_column_result r;
        r.code = t.stop_code ? t.stop_code : elements_code(t.n_items, o.have(), o.capacity);
        r.flags = 0;
        r.n_rows = t.n_rows;
        r.n_arrays = t.n_containers;
        r.n_elements = t.n_items;
        r.n_other = t.n_other;
        r.n_no_bits = 0;  // (items_emit's)
        *o.result = r;
        if (o.elements_select) *o.elements_select = items_select(r.code, t.n_items);
    }
};

}  // namespace msj_aelem

extern "C" uint64_t msj_array_elements_workspace_bytes(uint64_t n, uint64_t capacity) { return msj_rows::work_bytes(n, capacity); }

extern "C" int msj_launch_array_elements(const msj_token_view &t, const msj_number_view &nv, const msj_field *d_rows,
                                         const msj_select_documents_result *d_rows_select, uint64_t *d_offsets, uint8_t *d_valid,
                                         uint64_t capacity, msj_field *d_elements, uint64_t elements_capacity, msj_array_column_result *d_result,
                                         msj_select_documents_result *d_elements_select, void *d_ws, void *stream) {
    using msj_aelem::Elements;
    return msj_rows::launch_items<Elements>(t, nv, d_rows, d_rows_select, d_offsets, d_valid, capacity,
                                            Elements::Out{d_elements, elements_capacity, d_result, d_elements_select}, d_ws, stream);
}
