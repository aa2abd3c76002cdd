// knn_index_dev.h -- the device-side door into knn_index.hip: the tree walk as a function a kernel of another file can end with its own
// epilogue (ground.hip's normals), and a build that takes its points and their count from device memory, so that a caller can go from a
// compaction to the queries without a trip through the host.  Internal; the public lio_knn_index_* contract (host arrays, 1 <= k <= 8) is
// unchanged.  The rules are the index's: d2 = ((dx*dx) + dy*dy) + dz*dz in f32, separately rounded; ties go to the smaller index.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lio {
namespace knn_index {

constexpr uint32_t kLeaf = 32;           // points per leaf
constexpr uint32_t kNone = 0xFFFFFFFFu;  // an empty result slot

// lower bound of the f32 distance from q to any point of the box; `empty` for the padding boxes; *mid = squared distance to the box's centre
// (visiting order only)
__device__ __forceinline__ float box_bound(const float4* __restrict__ nodes, uint32_t node, float qx, float qy, float qz, bool* empty, float* mid) {
    const float4 lo = nodes[2ull * node], hi = nodes[2ull * node + 1];
    *empty = lo.x > hi.x;
    const float cx = (lo.x + hi.x) * 0.5f - qx, cy = (lo.y + hi.y) * 0.5f - qy, cz = (lo.z + hi.z) * 0.5f - qz;
    *mid = cx * cx + cy * cy + cz * cz;
    const float gx = fmaxf(fmaxf(lo.x - qx, qx - hi.x), 0.f);
    const float gy = fmaxf(fmaxf(lo.y - qy, qy - hi.y), 0.f);
    const float gz = fmaxf(fmaxf(lo.z - qz, qz - hi.z), 0.f);
    return gx * gx + gy * gy + gz * gz;
}

template <int K>
__device__ __forceinline__ void consider(float d, uint32_t id, float (&kd)[K], uint32_t (&ki)[K]) {
    if (!(d < kd[K - 1] || (d == kd[K - 1] && id < ki[K - 1]))) return;
#pragma unroll
    for (int s = 0; s < K; s++) {  // insertion: the candidate sinks to its place, the slots behind it move one down, the last drops out
        const bool lt = d < kd[s] || (d == kd[s] && id < ki[s]);
        const float td = kd[s];
        const uint32_t ti = ki[s];
        kd[s] = lt ? d : td;
        ki[s] = lt ? id : ti;
        d = lt ? td : d;
        id = lt ? ti : id;
    }
}

// the K nearest of the nf indexed points to the finite query (qx, qy, qz) into kd / ki (initialised to +inf / kNone by the caller), ascending
// (d2, index): one lane walks the tree nearer child first without a stack (the path is the node index, one bit per level says whether the
// lane is in the far child).  This is kx_query's loop word for word (knn_index.hip keeps its own copy inline, whose code the compiler
// lays out differently): a change to one belongs in the other.
template <int K>
__device__ __forceinline__ void walk(float qx, float qy, float qz, const float4* __restrict__ nodes, const float4* __restrict__ leaves, uint32_t nf,
                                     uint32_t P, int L, float (&kd)[K], uint32_t (&ki)[K]) {
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

// How many of the nf indexed points lie within r2 (d2 <= r2) of the finite query, counted up to `need`: the same stackless path as walk<K>
// (node index + one far bit per level, nearer child first, box_bound as the lower bound), but bounded from the root -- a box is entered
// iff its bound is <= r2, whatever was found so far -- and left for good once `need` points are counted.  count >= need is exactly
// walk<need>'s test kd[need - 1] <= r2: both ask whether `need` points have an f32 distance of at most r2.
__device__ __forceinline__ uint32_t walk_radius(float qx, float qy, float qz, const float4* __restrict__ nodes, const float4* __restrict__ leaves,
                                                uint32_t nf, uint32_t P, int L, float r2, uint32_t need) {
    uint32_t node = 1, far = 0, found = 0;
    int lvl = 0;
    bool down = true;
    while (true) {
        if (down) {
            if (lvl == L) {
                const uint32_t a = (node - P) * kLeaf, cnt = a < nf ? min(kLeaf, nf - a) : 0u;
                for (uint32_t t0 = 0; t0 < cnt; t0 += 8) {
                    float4 p[8];
#pragma unroll
                    for (int u = 0; u < 8; u++) p[u] = leaves[a + min(t0 + u, cnt - 1u)];
#pragma unroll
                    for (int u = 0; u < 8; u++) {
                        const float dx = p[u].x - qx, dy = p[u].y - qy, dz = p[u].z - qz;
                        found += (t0 + u < cnt && dx * dx + dy * dy + dz * dz <= r2) ? 1u : 0u;
                    }
                    if (found >= need) return found;
                }
                down = false;
            } else {
                bool e0, e1;
                float m0, m1;
                const uint32_t c0 = 2 * node;
                const float b0 = box_bound(nodes, c0, qx, qy, qz, &e0, &m0), b1 = box_bound(nodes, c0 + 1, qx, qy, qz, &e1, &m1);
                const bool right = e0 || (!e1 && (b1 < b0 || (b1 == b0 && m1 < m0)));
                const bool ne = right ? e1 : e0;
                const float nb = right ? b1 : b0;
                if (ne || nb > r2) {
                    down = false;  // neither child can hold a point within the radius
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
                if (!es && !(bs > r2)) {
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
    return found;
}

// A tree over points that are already on the device, their count there too.  The caller owns the handle; reserve() grows it geometrically
// and build() allocates nothing.  The tree is sized by n_max (the count's upper bound, known to the host): the leaf slots past the last
// point hold empty boxes, which the walk passes by.  After build(), leaves[0 .. *d_n) are the points in Morton order, so a self-query runs
// one lane per leaf point and needs no query sort.
struct DeviceIndex {
    uint64_t cap = 0;  // points the buffers hold
    float4* leaves = nullptr;
    float4* nodes = nullptr;  // 2 x 2P float4 (P <= the power of two above cap / kLeaf)
    float* box = nullptr;
    float* parts = nullptr;
    uint32_t *klo = nullptr, *khi = nullptr, *vals = nullptr, *kb = nullptr, *vb = nullptr, *scratch = nullptr;
    uint32_t P = 0;  // of the last build
    int L = 0;
};
int device_index_reserve(DeviceIndex& x, uint64_t n_max);
void device_index_free(DeviceIndex& x);
// pts: n_max slots of {x, y, z, index bits}, the first *d_n of them valid and finite (d_n = NULL: all n_max); everything on `st`.  The sort
// runs over the n_max slots, those past the count keyed ~0: they sort last and end in empty leaf boxes.
int device_index_build(hipStream_t st, DeviceIndex& x, const float4* pts, const uint32_t* d_n, uint32_t n_max);

}  // namespace knn_index
}  // namespace lio
