// Test-only harness: compiles mojo_simdjson_amd/csrc/number_math.h for the host (g++), so that the number conversion of
// msj_number_values_device (csrc/numbers_kernel.hip) -- scan, Clinger, Eisel-Lemire and the exact big-integer path, the
// same code the kernels run -- is checked against Python on a CPU-only box.  NOT part of the product.
#include "../mojo_simdjson_amd/csrc/number_math.h"

using namespace msj::num;

extern "C" {

// one number at buf[start]: kind (MSJ_NUMBER_*), bits; returns the path (0 fast, 1 Eisel-Lemire, 2 exact)
uint32_t nm_convert(const uint8_t *buf, uint64_t len, uint64_t start, uint64_t *bits, uint32_t *kind) {
    const SerialRuns r{buf, len};
    const Result res = convert(r, start);
    *bits = res.bits;
    *kind = res.kind;
    return res.path;
}

// many numbers of one buffer; paths[0..2] count the paths taken
void nm_convert_batch(const uint8_t *buf, uint64_t len, const uint64_t *starts, uint64_t n, uint64_t *bits, uint32_t *kinds,
                      uint64_t *paths) {
    const SerialRuns r{buf, len};
    for (uint64_t i = 0; i < n; i++) {
        const Result res = convert(r, starts[i]);
        bits[i] = res.bits;
        kinds[i] = res.kind;
        paths[res.path]++;
    }
}

void nm_pow5(int32_t q, uint64_t *out) {
    out[0] = msj::kPow5[q - msj::kPow5Min][0];
    out[1] = msj::kPow5[q - msj::kPow5Min][1];
}
int32_t nm_floor_log2_pow5(int32_t q) { return floor_log2_pow5(q); }

}  // extern "C"
