// knn_index.hip -- exact k nearest neighbours over a static cloud on gfx950 (wave64): the pcl::KdTreeFLANN<PointXYZRGB> of texture_mesh
// (slam/src/graph_utils.cpp:449-501), as an implicit bounding-volume tree over Morton-ordered leaves.
//
//   expand    xyz (n x 3) -> float4 {x, y, z, input index bits} + the finite points per tile
//   compact   device_prims.h's stable compaction of the finite points (PCL's isFinite filter; input order kept)
//   bbox      per-workgroup records (grid-stride) -> one workgroup folds them
//   morton    63-bit key per point, 21 bits per axis over the finite box, as a low and a high word
//   sort      four 8-bit passes by the low word, a gather of the high word, four passes by the high word (cloud.hip's stable radix pass)
//   leaves    kLeaf consecutive sorted points per leaf, gathered as float4 {x, y, z, index bits}, and one AABB per leaf
//   levels    a complete binary tree in heap order over the leaves (padded to a power of two with empty boxes), eight levels per launch
//             folded in LDS
//   query     the queries Morton-sorted the same way; one lane per query walks the tree nearer child first without a stack (the path is the
//             node index, one bit per level says whether the lane is in the far child), the top k in registers ordered by (d2, index);
//             knn_index_dev.h holds the same walk as a function for kernels of other files (kept apart from this kernel's own loop: inlined
//             from a function the compiler lays it out with more branches and two more registers) and declares the build, which takes its
//             point count from the host (lio_knn_index_build, after the compaction) or from device memory (ground.hip)
//
// Exactness: a point's distance is ((dx*dx) + dy*dy) + dz*dz in f32 (d = p - q, no contraction: -ffp-contract=off); a box's bound is the same
// expression over the clamped per-axis gaps max(lo - q, q - hi, 0).  Rounding is monotone, so the bound never exceeds the distance of a point
// inside the box; a box is skipped only when its bound is STRICTLY greater than the current k-th distance (at equality a smaller index can still
// win).  Ties at equal f32 distance go to the smaller input index -- the project's rule (FLANN's order depends on its tree).
// Workgroups hand results to each other only at kernel boundaries.  Point indices are 32-bit (PCL's int: 2^31 - 1 points), byte offsets 64-bit.
#include <algorithm>
#include <vector>

#include "device_prims.h"
#include "knn_index_dev.h"

namespace lio {
namespace knn_index {

using namespace prims;

constexpr uint32_t kBoxBlocks = 1024;          // workgroups of the bbox's first level
constexpr int kFold = 8;                       // tree levels per fold launch (256 nodes -> 1)
constexpr uint64_t kQueryChunk = 1ull << 22;   // queries per device pass (bounds the query scratch)

// every input point as {x, y, z, index bits}, and the finite ones per tile
__global__ __launch_bounds__(kThreads) void kx_expand(const float* __restrict__ xyz, uint32_t n, float4* __restrict__ pts, uint32_t* __restrict__ counts) {
    const uint32_t base = blockIdx.x * kTile;
    uint32_t c = 0;
#pragma unroll
    for (int r = 0; r < kItems; r++) {
        const uint32_t i = base + r * kThreads + threadIdx.x;
        if (i < n) {
            const float x = xyz[3ull * i], y = xyz[3ull * i + 1], z = xyz[3ull * i + 2];
            pts[i] = make_float4(x, y, z, __uint_as_float(i));
            c += finite3(x, y, z) ? 1u : 0u;
        }
    }
    compact_tile_count(c, counts);
}

// stable compaction of the finite points (input order kept)
__global__ __launch_bounds__(kThreads) void kx_compact(const float4* __restrict__ pts, uint32_t n, const uint32_t* __restrict__ offs, float4* __restrict__ out) {
    const uint32_t base = blockIdx.x * kTile;
    float4 p[kItems];
    bool fin[kItems];
#pragma unroll
    for (int r = 0; r < kItems; r++) {
        const uint32_t i = base + r * kThreads + threadIdx.x;
        p[r] = pts[i < n ? i : n - 1u];
        fin[r] = i < n && finite3(p[r].x, p[r].y, p[r].z);
    }
    compact_tile_write(fin, offs, [&](int r, uint32_t o) { out[o] = p[r]; });
}

// The build's kernels take the point count as (d_n, n_max): *d_n when d_n is given (a count that never left the device, n_max its upper
// bound), else n_max itself.

// bbox of the n finite points, level 1: one record {min x y z, max x y z} per workgroup (grid-stride)
__global__ __launch_bounds__(kThreads) void kx_box_part(const float4* __restrict__ p, const uint32_t* __restrict__ d_n, uint32_t n_max, float* __restrict__ parts) {
    const uint32_t n = d_n ? *d_n : n_max;
    float v[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (uint32_t i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads) {
        const float4 q = p[i];
        v[0] = fminf(v[0], q.x); v[1] = fminf(v[1], q.y); v[2] = fminf(v[2], q.z);
        v[3] = fmaxf(v[3], q.x); v[4] = fmaxf(v[4], q.y); v[5] = fmaxf(v[5], q.z);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int a = 0; a < 6; a++) v[a] = a < 3 ? fminf(v[a], __shfl_xor(v[a], off)) : fmaxf(v[a], __shfl_xor(v[a], off));
    __shared__ float red[kWaves][6];
    if ((threadIdx.x & 63) == 0)
        for (int a = 0; a < 6; a++) red[threadIdx.x >> 6][a] = v[a];
    __syncthreads();
    if (threadIdx.x < 6) {
        const int a = threadIdx.x;
        float r = red[0][a];
        for (int w = 1; w < kWaves; w++) r = a < 3 ? fminf(r, red[w][a]) : fmaxf(r, red[w][a]);
        parts[6u * blockIdx.x + a] = r;
    }
}

// level 2: one workgroup folds the records into box[6]
__global__ __launch_bounds__(kThreads) void kx_box_fold(const float* __restrict__ parts, uint32_t nparts, float* __restrict__ box) {
    __shared__ float red[kWaves][6];
    float v[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (uint32_t b = threadIdx.x; b < nparts; b += kThreads)
        for (int a = 0; a < 6; a++) v[a] = a < 3 ? fminf(v[a], parts[6u * b + a]) : fmaxf(v[a], parts[6u * b + a]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int a = 0; a < 6; a++) v[a] = a < 3 ? fminf(v[a], __shfl_xor(v[a], off)) : fmaxf(v[a], __shfl_xor(v[a], off));
    if ((threadIdx.x & 63) == 0)
        for (int a = 0; a < 6; a++) red[threadIdx.x >> 6][a] = v[a];
    __syncthreads();
    if (threadIdx.x < 6) {
        const int a = threadIdx.x;
        float r = red[0][a];
        for (int w = 1; w < kWaves; w++) r = a < 3 ? fminf(r, red[w][a]) : fmaxf(r, red[w][a]);
        box[a] = r;
    }
}

__device__ __forceinline__ uint64_t spread3(uint32_t a) {  // the 21 low bits of a to every third bit
    uint64_t x = a & 0x1FFFFFu;
    x = (x | x << 32) & 0x1F00000000FFFFull;
    x = (x | x << 16) & 0x1F0000FF0000FFull;
    x = (x | x << 8) & 0x100F00F00F00F00Full;
    x = (x | x << 4) & 0x10C30C30C30C30C3ull;
    x = (x | x << 2) & 0x1249249249249249ull;
    return x;
}
__device__ __forceinline__ uint32_t quant21(float v, float lo, float hi) {
    const float ext = hi - lo;
    float t = ext > 0.f ? (v - lo) * (2097151.0f / ext) : 0.f;
    t = fminf(fmaxf(t, 0.f), 2097151.0f);
    return (uint32_t)t;
}
__device__ __forceinline__ uint64_t morton(float x, float y, float z, const float* b) {
    return spread3(quant21(x, b[0], b[3])) | (spread3(quant21(y, b[1], b[4])) << 1) | (spread3(quant21(z, b[2], b[5])) << 2);
}

// keys of the n points of the index (the slots from n to n_max: ~0, behind every point); vals = their positions
__global__ __launch_bounds__(kThreads) void kx_keys_points(const float4* __restrict__ p, const uint32_t* __restrict__ d_n, uint32_t n_max,
                                                           const float* __restrict__ box, uint32_t* __restrict__ klo, uint32_t* __restrict__ khi,
                                                           uint32_t* __restrict__ vals) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n_max) return;
    uint64_t k = ~0ull;
    if (i < (d_n ? *d_n : n_max)) {
        const float4 q = p[i];
        k = morton(q.x, q.y, q.z, box);
    }
    klo[i] = (uint32_t)k;
    khi[i] = (uint32_t)(k >> 32);
    vals[i] = i;
}

// keys of the queries over the index's box (clamped to it); non-finite queries sort last
__global__ __launch_bounds__(kThreads) void kx_keys_queries(const float* __restrict__ q, uint32_t m, const float* __restrict__ box, uint32_t* __restrict__ klo,
                                                            uint32_t* __restrict__ khi, uint32_t* __restrict__ vals) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= m) return;
    const float x = q[3ull * i], y = q[3ull * i + 1], z = q[3ull * i + 2];
    const uint64_t k = finite3(x, y, z) ? morton(x, y, z, box) : ~0ull;
    klo[i] = (uint32_t)k;
    khi[i] = (uint32_t)(k >> 32);
    vals[i] = i;
}

__global__ __launch_bounds__(kThreads) void kx_gather_u32(const uint32_t* __restrict__ src, const uint32_t* __restrict__ idx, uint32_t n, uint32_t* __restrict__ dst) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i < n) dst[i] = src[idx[i]];
}

// the n points into sorted order (the stable sort keeps them, whose keys are below ~0 or equal to it at a smaller position, first)
__global__ __launch_bounds__(kThreads) void kx_gather_points(const float4* __restrict__ src, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ d_n,
                                                             uint32_t n_max, float4* __restrict__ dst) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i < (d_n ? *d_n : n_max)) dst[i] = src[idx[i]];
}

// one AABB per leaf slot l < P at heap node P + l (nodes[2 i] = lo, nodes[2 i + 1] = hi); slots past the last leaf get the empty box
// (lo = +inf > hi = -inf)
__global__ __launch_bounds__(kThreads) void kx_leaf_boxes(const float4* __restrict__ leaves, const uint32_t* __restrict__ d_n, uint32_t n_max, uint32_t P,
                                                          float4* __restrict__ nodes) {
    const uint32_t l = blockIdx.x * kThreads + threadIdx.x;
    if (l >= P) return;
    const uint32_t nf = d_n ? *d_n : n_max, nl = (nf + kLeaf - 1) / kLeaf;
    float4 lo = make_float4(INFINITY, INFINITY, INFINITY, 0.f), hi = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.f);
    if (l < nl) {
        const uint32_t a = l * kLeaf, b = min(a + kLeaf, nf);
        for (uint32_t j = a; j < b; j++) {
            const float4 p = leaves[j];
            lo.x = fminf(lo.x, p.x); lo.y = fminf(lo.y, p.y); lo.z = fminf(lo.z, p.z);
            hi.x = fmaxf(hi.x, p.x); hi.y = fmaxf(hi.y, p.y); hi.z = fmaxf(hi.z, p.z);
        }
    }
    nodes[2ull * (P + l)] = lo;
    nodes[2ull * (P + l) + 1] = hi;
}

// `levels` levels of the tree above the level whose first node is `first` (= 2^L, 2^L nodes): every workgroup folds 256 of its nodes (fewer
// near the root) in LDS and writes each level it makes
__global__ __launch_bounds__(kThreads) void kx_fold(float4* __restrict__ nodes, uint32_t first, int levels) {
    __shared__ float4 slo[kThreads], shi[kThreads];
    const uint32_t cnt = min(first, (uint32_t)kThreads);
    const uint32_t b0 = first + blockIdx.x * cnt;  // first child node of this workgroup
    const uint32_t t = threadIdx.x;
    if (t < cnt) {
        slo[t] = nodes[2ull * (b0 + t)];
        shi[t] = nodes[2ull * (b0 + t) + 1];
    }
    __syncthreads();
    uint32_t w = cnt, base = b0;
    for (int s = 0; s < levels; s++) {
        w >>= 1;
        base >>= 1;
        float4 lo, hi;
        if (t < w) {
            const float4 l0 = slo[2 * t], l1 = slo[2 * t + 1], h0 = shi[2 * t], h1 = shi[2 * t + 1];
            lo = make_float4(fminf(l0.x, l1.x), fminf(l0.y, l1.y), fminf(l0.z, l1.z), 0.f);
            hi = make_float4(fmaxf(h0.x, h1.x), fmaxf(h0.y, h1.y), fmaxf(h0.z, h1.z), 0.f);
        }
        __syncthreads();
        if (t < w) {
            slo[t] = lo;
            shi[t] = hi;
            nodes[2ull * (base + t)] = lo;
            nodes[2ull * (base + t) + 1] = hi;
        }
        __syncthreads();
    }
}

// one lane per query, in Morton order (perm); results go to the query's own position.  COLOUR: the floor-mean of the r, g, b bytes of the
// (up to) K neighbours packed as 0x00RRGGBB; otherwise the K (index, d2) pairs, ascending (d2, index), empty slots (-1, +inf).
template <int K, bool COLOUR>
__global__ __launch_bounds__(kThreads) void kx_query(const float* __restrict__ q, uint32_t m, const uint32_t* __restrict__ perm, const float4* __restrict__ nodes,
                                                     const float4* __restrict__ leaves, uint32_t nf, uint32_t P, int L, const uint32_t* __restrict__ rgb,
                                                     int32_t* __restrict__ oidx, float* __restrict__ od2, uint32_t* __restrict__ ocol) {
    const uint32_t j = blockIdx.x * kThreads + threadIdx.x;
    if (j >= m) return;
    const uint32_t qi = perm[j];
    const float qx = q[3ull * qi], qy = q[3ull * qi + 1], qz = q[3ull * qi + 2];
    float kd[K];
    uint32_t ki[K];
#pragma unroll
    for (int s = 0; s < K; s++) { kd[s] = INFINITY; ki[s] = kNone; }
    if (nf > 0 && finite3(qx, qy, qz)) {
        uint32_t node = 1, far = 0;  // far: bit l set = the path's node at level l is the far child of its parent
        int lvl = 0;
        bool down = true;
        while (true) {
            if (down) {
                if (lvl == L) {
                    const uint32_t a = (node - P) * kLeaf, cnt = min(kLeaf, nf - a);
                    for (uint32_t t0 = 0; t0 < cnt; t0 += 8) {
                        float4 p[8];
    #pragma unroll
                        for (int u = 0; u < 8; u++) p[u] = leaves[a + min(t0 + u, cnt - 1u)];
    #pragma unroll
                        for (int u = 0; u < 8; u++) {
                            if (t0 + u >= cnt) break;
                            const float dx = p[u].x - qx, dy = p[u].y - qy, dz = p[u].z - qz;
                            consider<K>(dx * dx + dy * dy + dz * dz, __float_as_uint(p[u].w), kd, ki);
                        }
                    }
                    down = false;
                } else {
                    bool e0, e1;
                    float m0, m1;
                    const uint32_t c0 = 2 * node;
                    const float b0 = box_bound(nodes, c0, qx, qy, qz, &e0, &m0), b1 = box_bound(nodes, c0 + 1, qx, qy, qz, &e1, &m1);
                    // nearer bound first; equal bounds (typically 0: q inside both boxes) by the distance to the box centres -- the order only
                    // decides how soon the k-th distance shrinks, never what is found
                    const bool right = e0 || (!e1 && (b1 < b0 || (b1 == b0 && m1 < m0)));
                    const bool ne = right ? e1 : e0;
                    const float nb = right ? b1 : b0;
                    if (ne || nb > kd[K - 1]) {
                        down = false;  // the far child is empty or no nearer
                    } else {
                        node = c0 + (right ? 1u : 0u);
                        lvl++;
                        far &= ~(1u << lvl);
                    }
                }
            } else {
                if (lvl == 0) break;
                if (!((far >> lvl) & 1u)) {
                    bool es;
                    float ms;
                    const uint32_t sib = node ^ 1u;
                    const float bs = box_bound(nodes, sib, qx, qy, qz, &es, &ms);
                    if (!es && !(bs > kd[K - 1])) {
                        node = sib;
                        far |= 1u << lvl;
                        down = true;
                        continue;
                    }
                }
                node >>= 1;
                lvl--;
            }
        }
    }
    if (COLOUR) {
        uint32_t r = 0, g = 0, b = 0, c = 0;
#pragma unroll
        for (int s = 0; s < K; s++)
            if (ki[s] != kNone) {
                const uint32_t w = rgb[ki[s]];
                r += (w >> 16) & 255u;
                g += (w >> 8) & 255u;
                b += w & 255u;
                c++;
            }
        ocol[qi] = c ? ((r / c) << 16) | ((g / c) << 8) | (b / c) : 0u;
    } else {
#pragma unroll
        for (int s = 0; s < K; s++) {
            oidx[(uint64_t)qi * K + s] = ki[s] == kNone ? -1 : (int32_t)ki[s];
            od2[(uint64_t)qi * K + s] = kd[s];
        }
    }
}

template <bool COLOUR>
void launch_query(int k, hipStream_t st, const float* q, uint32_t m, const uint32_t* perm, const float4* nodes, const float4* leaves, uint32_t nf, uint32_t P,
                  int L, const uint32_t* rgb, int32_t* oidx, float* od2, uint32_t* ocol) {
    const dim3 g((m + kThreads - 1) / kThreads), b(kThreads);
    switch (k) {
#define KX_CASE(KK) \
    case KK: kx_query<KK, COLOUR><<<g, b, 0, st>>>(q, m, perm, nodes, leaves, nf, P, L, rgb, oidx, od2, ocol); break;
        KX_CASE(1) KX_CASE(2) KX_CASE(3) KX_CASE(4) KX_CASE(5) KX_CASE(6) KX_CASE(7) KX_CASE(8)
#undef KX_CASE
        default: break;
    }
}

// device allocations of one call, freed when it returns
struct Temps {
    std::vector<void*> p;
    ~Temps() {
        for (void* x : p) (void)hipFree(x);
    }
    template <typename T>
    T* get(uint64_t count) {
        void* x = nullptr;
        if (hipMalloc(&x, std::max<uint64_t>(count, 1) * sizeof(T)) != hipSuccess) {
            (void)hipGetLastError();
            set_error("lio_knn_index: %llu bytes of device memory not available", (unsigned long long)(count * sizeof(T)));
            return nullptr;
        }
        p.push_back(x);
        return static_cast<T*>(x);
    }
};

// the Morton order of n keys (63 bits as low / high words): four passes by the low word, the high word gathered into that order, four
// passes by it.  klo / vals hold the input and are overwritten; returns the permutation (a pointer to vals or vb).
int morton_sort(hipStream_t st, uint32_t* klo, const uint32_t* khi, uint32_t* vals, uint32_t* kb, uint32_t* vb, uint32_t n, uint32_t* scratch, uint32_t** perm) {
    uint32_t *ka = klo, *va = vals;
    for (int p = 0; p < 4; p++) {
        const int rc = cloud::radix_pass(st, ka, va, kb, vb, n, 8 * p, scratch);
        if (rc != LIO_OK) return rc;
        std::swap(ka, kb);
        std::swap(va, vb);
    }
    kx_gather_u32<<<dim3(blocks_of(n)), dim3(kThreads), 0, st>>>(khi, va, n, ka);  // (four passes: the order is back in klo / vals)
    LIO_HIP_TRY(hipGetLastError());
    for (int p = 0; p < 4; p++) {
        const int rc = cloud::radix_pass(st, ka, va, kb, vb, n, 8 * p, scratch);
        if (rc != LIO_OK) return rc;
        std::swap(ka, kb);
        std::swap(va, vb);
    }
    *perm = va;
    return LIO_OK;
}

// ---- the build (knn_index_dev.h) ----
static uint32_t leaf_slots(uint64_t n, int* L) {
    const uint32_t nl = (uint32_t)((std::max<uint64_t>(n, 1) + kLeaf - 1) / kLeaf);
    int l = 0;
    while ((1u << l) < nl) l++;
    *L = l;
    return 1u << l;
}

void device_index_free(DeviceIndex& x) {
    void* all[] = {x.leaves, x.nodes, x.box, x.parts, x.klo, x.khi, x.vals, x.kb, x.vb, x.scratch};
    for (void* p : all)
        if (p) (void)hipFree(p);
    x = DeviceIndex();
}

int device_index_reserve(DeviceIndex& x, uint64_t n_max) {
    if (n_max <= x.cap) return LIO_OK;
    if (n_max > 0x7FFFFFFFull) { set_error("knn index: %llu points exceed the int index range (2^31 - 1)", (unsigned long long)n_max); return LIO_E_CAPACITY; }
    const uint64_t want = std::min<uint64_t>(std::max<uint64_t>(n_max, std::max<uint64_t>(2 * x.cap, 1ull << 16)), 0x7FFFFFFFull);
    device_index_free(x);
    int L = 0;
    const uint32_t P = leaf_slots(want, &L);
    bool ok = hipMalloc(&x.leaves, want * sizeof(float4)) == hipSuccess && hipMalloc(&x.nodes, 4ull * P * sizeof(float4)) == hipSuccess &&
              hipMalloc(&x.box, 8 * sizeof(float)) == hipSuccess && hipMalloc(&x.parts, 6ull * kBoxBlocks * sizeof(float)) == hipSuccess &&
              hipMalloc(&x.scratch, cloud::radix_scratch_words(want) * sizeof(uint32_t)) == hipSuccess;
    uint32_t** w[] = {&x.klo, &x.khi, &x.vals, &x.kb, &x.vb};
    for (uint32_t** p : w) ok = ok && hipMalloc(p, want * sizeof(uint32_t)) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        device_index_free(x);
        set_error("knn index: device memory for a tree over %llu points not available", (unsigned long long)want);
        return LIO_E_DEVICE;
    }
    x.cap = want;
    return LIO_OK;
}

int device_index_build(hipStream_t st, DeviceIndex& x, const float4* pts, const uint32_t* d_n, uint32_t n_max) {
    if (n_max == 0 || n_max > x.cap) return LIO_E_INVALID;
    const uint32_t nb = std::min<uint32_t>(blocks_of(n_max), kBoxBlocks);
    kx_box_part<<<dim3(nb), dim3(kThreads), 0, st>>>(pts, d_n, n_max, x.parts);
    kx_box_fold<<<dim3(1), dim3(kThreads), 0, st>>>(x.parts, nb, x.box);
    kx_keys_points<<<dim3(blocks_of(n_max)), dim3(kThreads), 0, st>>>(pts, d_n, n_max, x.box, x.klo, x.khi, x.vals);
    LIO_HIP_TRY(hipGetLastError());
    uint32_t* perm = nullptr;
    const int rc = morton_sort(st, x.klo, x.khi, x.vals, x.kb, x.vb, n_max, x.scratch, &perm);
    if (rc != LIO_OK) return rc;
    kx_gather_points<<<dim3(blocks_of(n_max)), dim3(kThreads), 0, st>>>(pts, perm, d_n, n_max, x.leaves);
    x.P = leaf_slots(n_max, &x.L);
    kx_leaf_boxes<<<dim3(blocks_of(x.P)), dim3(kThreads), 0, st>>>(x.leaves, d_n, n_max, x.P, x.nodes);
    LIO_HIP_TRY(hipGetLastError());
    for (int lv = x.L; lv > 0;) {
        const int f = std::min(lv, kFold);
        const uint32_t first = 1u << lv;
        kx_fold<<<dim3(std::max<uint32_t>(1u, first / kThreads)), dim3(kThreads), 0, st>>>(x.nodes, first, f);
        lv -= f;
    }
    LIO_HIP_TRY(hipGetLastError());
    return LIO_OK;
}

}  // namespace knn_index
}  // namespace lio

using namespace lio;
using namespace lio::knn_index;

struct lio_knn_index {
    int device;
    hipStream_t stream;
    hipEvent_t ev[2];
    float4* leaves;  // nf points in Morton order, {x, y, z, input index bits}
    float4* nodes;   // 2 x 2P float4: the heap-ordered AABBs (node 0 unused)
    uint32_t* rgb;   // n packed colours in input order (NULL: built without)
    float* box;      // the finite box, 6 floats
    uint64_t n;
    uint32_t nf, nl, P;
    int L;
    double build_us, query_us;
};

namespace {

void release(lio_knn_index* x) {
    if (x->leaves) (void)hipFree(x->leaves);
    if (x->nodes) (void)hipFree(x->nodes);
    if (x->rgb) (void)hipFree(x->rgb);
    x->leaves = x->nodes = nullptr;
    x->rgb = nullptr;
    x->n = x->nf = x->nl = x->P = 0;
    x->L = 0;
}

// the k nearest of m host queries: (idx, d2) when rgb_out is NULL, else the colours
int run_query(lio_knn_index* x, const float* q, uint64_t m, int k, int32_t* idx, float* d2, uint8_t* rgb_out) {
    x->query_us = 0;
    if (m == 0) return LIO_OK;
    hipSetDevice(x->device);
    const bool colour = rgb_out != nullptr;
    if (x->nf == 0) {  // nothing indexed: every slot empty
        for (uint64_t i = 0; i < m; i++) {
            if (colour) {
                rgb_out[3 * i] = rgb_out[3 * i + 1] = rgb_out[3 * i + 2] = 0;
            } else {
                for (int s = 0; s < k; s++) { idx[i * k + s] = -1; d2[i * k + s] = INFINITY; }
            }
        }
        return LIO_OK;
    }
    const uint64_t chunk = std::min<uint64_t>(m, kQueryChunk);
    Temps T;
    float* dq = T.get<float>(3 * chunk);
    uint32_t *klo = T.get<uint32_t>(chunk), *khi = T.get<uint32_t>(chunk), *vals = T.get<uint32_t>(chunk), *kb = T.get<uint32_t>(chunk), *vb = T.get<uint32_t>(chunk);
    uint32_t* scratch = T.get<uint32_t>(cloud::radix_scratch_words(chunk));
    int32_t* oidx = colour ? nullptr : T.get<int32_t>(chunk * k);
    float* od2 = colour ? nullptr : T.get<float>(chunk * k);
    uint32_t* ocol = colour ? T.get<uint32_t>(chunk) : nullptr;
    if (!dq || !klo || !khi || !vals || !kb || !vb || !scratch || (colour ? !ocol : (!oidx || !od2))) return LIO_E_DEVICE;
    std::vector<uint32_t> hcol(colour ? chunk : 0);
    double total = 0;
    for (uint64_t q0 = 0; q0 < m; q0 += chunk) {
        const uint32_t mc = (uint32_t)std::min<uint64_t>(chunk, m - q0);
        LIO_HIP_TRY(hipMemcpyAsync(dq, q + 3 * q0, 3ull * mc * sizeof(float), hipMemcpyHostToDevice, x->stream));
        LIO_HIP_TRY(hipEventRecord(x->ev[0], x->stream));
        kx_keys_queries<<<dim3(blocks_of(mc)), dim3(kThreads), 0, x->stream>>>(dq, mc, x->box, klo, khi, vals);
        LIO_HIP_TRY(hipGetLastError());
        uint32_t* perm = nullptr;
        const int rc = morton_sort(x->stream, klo, khi, vals, kb, vb, mc, scratch, &perm);
        if (rc != LIO_OK) return rc;
        if (colour)
            launch_query<true>(k, x->stream, dq, mc, perm, x->nodes, x->leaves, x->nf, x->P, x->L, x->rgb, nullptr, nullptr, ocol);
        else
            launch_query<false>(k, x->stream, dq, mc, perm, x->nodes, x->leaves, x->nf, x->P, x->L, nullptr, oidx, od2, nullptr);
        LIO_HIP_TRY(hipGetLastError());
        LIO_HIP_TRY(hipEventRecord(x->ev[1], x->stream));
        if (colour) {
            LIO_HIP_TRY(hipMemcpyAsync(hcol.data(), ocol, (uint64_t)mc * sizeof(uint32_t), hipMemcpyDeviceToHost, x->stream));
        } else {
            LIO_HIP_TRY(hipMemcpyAsync(idx + q0 * k, oidx, (uint64_t)mc * k * sizeof(int32_t), hipMemcpyDeviceToHost, x->stream));
            LIO_HIP_TRY(hipMemcpyAsync(d2 + q0 * k, od2, (uint64_t)mc * k * sizeof(float), hipMemcpyDeviceToHost, x->stream));
        }
        LIO_HIP_TRY(hipStreamSynchronize(x->stream));
        total += elapsed_us(x->ev[0], x->ev[1]);
        if (colour)
            for (uint32_t i = 0; i < mc; i++) {
                const uint32_t w = hcol[i];
                uint8_t* o = rgb_out + 3 * (q0 + i);
                o[0] = (uint8_t)(w >> 16);
                o[1] = (uint8_t)(w >> 8);
                o[2] = (uint8_t)w;
            }
    }
    x->query_us = total;
    return LIO_OK;
}

}  // namespace

extern "C" {

lio_knn_index* lio_knn_index_create(int device) {
    lio_knn_index* x = new lio_knn_index();
    memset(x, 0, sizeof(*x));
    x->device = device;
    if (!open_device("lio_knn_index_create", device, &x->stream, x->ev, 2)) {
        delete x;
        return nullptr;
    }
    if (!alloc(&x->box, 8)) {
        (void)hipGetLastError();
        set_error("lio_knn_index_create: stream / event / box allocation failed");
        lio_knn_index_destroy(x);
        return nullptr;
    }
    return x;
}

void lio_knn_index_destroy(lio_knn_index* x) {
    if (!x) return;
    hipSetDevice(x->device);
    if (x->stream) hipStreamSynchronize(x->stream);
    release(x);
    if (x->box) hipFree(x->box);
    for (int i = 0; i < 2; i++)
        if (x->ev[i]) hipEventDestroy(x->ev[i]);
    if (x->stream) hipStreamDestroy(x->stream);
    delete x;
}

int lio_knn_index_build(lio_knn_index* x, const float* xyz, const uint32_t* rgb, uint64_t n, uint64_t* n_finite) {
    if (!x || (!xyz && n)) return LIO_E_INVALID;
    if (n > 0x7FFFFFFFull) {
        set_error("lio_knn_index_build: %llu points exceed the int index range (2^31 - 1)", (unsigned long long)n);
        return LIO_E_CAPACITY;
    }
    hipSetDevice(x->device);
    release(x);
    x->build_us = 0;
    if (n_finite) *n_finite = 0;
    if (n == 0) return LIO_OK;
    const uint32_t nn = (uint32_t)n, ntiles = (uint32_t)tiles_of(n);
    Temps T;
    float* dxyz = T.get<float>(3 * n);
    float4* pts = T.get<float4>(n);
    float4* cpt = T.get<float4>(n);
    uint32_t* counts = T.get<uint32_t>(compact_words(n));
    float* parts = T.get<float>(6ull * kBoxBlocks);
    if (!dxyz || !pts || !cpt || !counts || !parts) return LIO_E_DEVICE;
    if (rgb && hipMalloc(&x->rgb, n * sizeof(uint32_t)) != hipSuccess) {
        (void)hipGetLastError();
        x->rgb = nullptr;
        set_error("lio_knn_index_build: %llu bytes of device memory not available for the colours", (unsigned long long)(n * 4));
        return LIO_E_DEVICE;
    }
    LIO_HIP_TRY(hipMemcpyAsync(dxyz, xyz, 3 * n * sizeof(float), hipMemcpyHostToDevice, x->stream));
    if (rgb) LIO_HIP_TRY(hipMemcpyAsync(x->rgb, rgb, n * sizeof(uint32_t), hipMemcpyHostToDevice, x->stream));
    LIO_HIP_TRY(hipEventRecord(x->ev[0], x->stream));
    // finite points, compacted in input order
    kx_expand<<<dim3(ntiles), dim3(kThreads), 0, x->stream>>>(dxyz, nn, pts, counts);
    LIO_HIP_TRY(hipGetLastError());
    const uint32_t* d_nf = compact_finish(x->stream, counts, n);
    if (!d_nf) return LIO_E_DEVICE;
    kx_compact<<<dim3(ntiles), dim3(kThreads), 0, x->stream>>>(pts, nn, counts, cpt);
    LIO_HIP_TRY(hipGetLastError());
    uint32_t nf = 0;
    LIO_HIP_TRY(hipMemcpyAsync(&nf, d_nf, sizeof(uint32_t), hipMemcpyDeviceToHost, x->stream));
    LIO_HIP_TRY(hipStreamSynchronize(x->stream));
    if (n_finite) *n_finite = nf;
    x->n = n;
    if (nf == 0) {
        LIO_HIP_TRY(hipEventRecord(x->ev[1], x->stream));
        LIO_HIP_TRY(hipStreamSynchronize(x->stream));
        x->build_us = elapsed_us(x->ev[0], x->ev[1]);
        return LIO_OK;
    }
    // the tree over exactly the nf compacted points: pts (n >= nf slots) becomes the leaves; the sort scratch lives for this call
    DeviceIndex d;
    d.cap = nf;
    d.leaves = pts;
    d.box = x->box;
    d.parts = parts;
    d.klo = T.get<uint32_t>(nf); d.khi = T.get<uint32_t>(nf); d.vals = T.get<uint32_t>(nf); d.kb = T.get<uint32_t>(nf); d.vb = T.get<uint32_t>(nf);
    d.scratch = T.get<uint32_t>(cloud::radix_scratch_words(nf));
    if (!d.klo || !d.khi || !d.vals || !d.kb || !d.vb || !d.scratch) return LIO_E_DEVICE;
    int L = 0;
    const uint32_t P = leaf_slots(nf, &L);
    if (!alloc(&x->nodes, 4ull * P)) {
        (void)hipGetLastError();
        x->nodes = nullptr;
        set_error("lio_knn_index_build: %llu bytes of device memory not available for the tree", (unsigned long long)(4ull * P * sizeof(float4)));
        return LIO_E_DEVICE;
    }
    d.nodes = x->nodes;
    const int rc = device_index_build(x->stream, d, cpt, nullptr, nf);
    if (rc != LIO_OK) return rc;
    LIO_HIP_TRY(hipEventRecord(x->ev[1], x->stream));
    LIO_HIP_TRY(hipStreamSynchronize(x->stream));
    x->build_us = elapsed_us(x->ev[0], x->ev[1]);
    // keep the leaves: take pts out of the temporaries
    T.p.erase(std::find(T.p.begin(), T.p.end(), (void*)pts));
    x->leaves = pts;
    x->nf = nf;
    x->nl = (nf + kLeaf - 1) / kLeaf;
    x->P = P;
    x->L = L;
    return LIO_OK;
}

int lio_knn_index_query(lio_knn_index* x, const float* q, uint64_t m, int k, int32_t* idx, float* d2) {
    if (!x || k < 1 || k > 8 || (m && (!q || !idx || !d2))) return LIO_E_INVALID;
    return run_query(x, q, m, k, idx, d2, nullptr);
}

int lio_knn_index_colour(lio_knn_index* x, const float* q, uint64_t m, int k, uint8_t* rgb_out) {
    if (!x || k < 1 || k > 8 || (m && (!q || !rgb_out))) return LIO_E_INVALID;
    if (x->nf && !x->rgb) {
        set_error("lio_knn_index_colour: the index was built without colours");
        return LIO_E_STATE;
    }
    return run_query(x, q, m, k, nullptr, nullptr, rgb_out);
}

int lio_knn_index_last_times(lio_knn_index* x, double* build_us, double* query_us) {
    if (!x) return LIO_E_INVALID;
    if (build_us) *build_us = x->build_us;
    if (query_us) *query_us = x->query_us;
    return LIO_OK;
}

}  // extern "C"
