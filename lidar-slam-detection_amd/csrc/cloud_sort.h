// cloud_sort.h -- the device-wide scan and the stable radix pass of cloud.hip, for the other files that sort (knn_index.hip, bev.hip), and the
// view of a lio_cloud's device points for the files that read a whole cloud (bev.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct lio_cloud;

namespace lio {
namespace cloud {

// device-wide exclusive prefix sum of m uint32 words in place; aux holds scan_aux_words(m) words
uint64_t scan_aux_words(uint64_t m);
int exclusive_scan(hipStream_t st, uint32_t* data, uint64_t m, uint32_t* aux);

// one stable pass of an LSD radix sort of (key, value) pairs by the 8-bit digit (key >> shift) & 255, kin/vin -> kout/vout (n <= 2^31 - 1);
// scratch holds radix_scratch_words(n) words
uint64_t radix_scratch_words(uint64_t n);
int radix_pass(hipStream_t st, const uint32_t* kin, const uint32_t* vin, uint32_t* kout, uint32_t* vout, uint32_t n, int shift, uint32_t* scratch);

// the points of a cloud as they lie on the device, and the stream its appends and voxel grid run on
struct CloudView {
    const float4* pts;
    uint64_t n;
    hipStream_t stream;
    int device;
};
CloudView cloud_view(const lio_cloud* c);

}  // namespace cloud
}  // namespace lio
