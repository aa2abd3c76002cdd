#!/usr/bin/env python3
"""Records tests/golden/voxelize.npz and voxelize_deviations.npz from the reference's own preprocess_kernel.cu and voxelization_kernel.cu
(sensor_driver/inference/voxelize/).

The two files are compiled FOR THE HOST, CPU only, with a generated shim that #includes them by path, into a TEMPORARY directory outside the
tree: /opt/rocm/llvm/bin/clang++ -O2 -ffp-contract=off -std=c++17 (it has _Float16).  Nothing compiled is kept.  The shim predefines the guards
of launch.cuh and check.hpp, makes cuda_linear_index a global and cuda_linear_launch a for loop that sets it -- the kernels run one thread
after another in index order, the execution include/lio_hip.h pins the device to -- maps the runtime's allocation and copy calls to calloc /
memset / memcpy (allocations padded: a call into a full window writes one row beyond max_points there) and gives atomicCAS / atomicAdd plain
bodies.  The call sequence is LidarInference::forward's (lidar_inference.cpp:81-85): n clamped to max_points, preprocess, voxelise.

Per case of tests/voxelize_cases.py and per call: the input (single-call cases), the motion, the window's counts (and its rows for cases of
several calls), the features as uint16, the indices, the counts, the number of voxels and the real number; per case the params and
compute_grid_size's grid.
Checked here: no case outside the deviation file holds a non-finite coordinate or a point that passes the grid test and fails the range test,
and the numpy restatement equals every recorded array of those cases.

    python tools/record_voxelize_golden.py [--reference /root/reference]
"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests")]
import voxelize_cases as vc  # noqa: E402

F = np.float32
CXX = "/opt/rocm/llvm/bin/clang++"
LAST_WINDOW_ONLY = ("window_400",)  # to keep the file small: every window depends on the ones before it

SHIM = r"""
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>
#define __LAUNCH_CUH__
#define __CHECK_HPP__
#define __device__
#define __global__
#define __host__
#define private public
typedef _Float16 half;
static inline half __float2half(float f) { return (half)f; }
struct uint4 { unsigned int x, y, z, w; };
static inline uint4 make_uint4(unsigned int x, unsigned int y, unsigned int z, unsigned int w) { uint4 r = {x, y, z, w}; return r; }
typedef void* cudaStream_t;
enum { cudaMemcpyHostToDevice, cudaMemcpyDeviceToHost };
static size_t cuda_linear_index;
#define cuda_linear_launch(kernel, stream, num, ...) \
    for (cuda_linear_index = 0; cuda_linear_index < (size_t)(num); cuda_linear_index++) kernel(num, __VA_ARGS__)
#define checkRuntime(call) (call)
#define Assertf(cond, fmt, ...) do { } while (0)
template <class T> static int cudaMalloc(T** p, size_t n) { *p = (T*)calloc(1, n + 65536); return 0; }
template <class T> static int cudaMallocHost(T** p, size_t n) { *p = (T*)calloc(1, n + 65536); return 0; }
static int cudaFree(void* p) { free(p); return 0; }
static int cudaFreeHost(void* p) { free(p); return 0; }
static int cudaMemsetAsync(void* p, int v, size_t n, cudaStream_t) { memset(p, v, n); return 0; }
static int cudaMemcpyAsync(void* d, const void* s, size_t n, int, cudaStream_t) { memcpy(d, s, n); return 0; }
static int cudaStreamSynchronize(cudaStream_t) { return 0; }
static inline unsigned int atomicCAS(unsigned int* a, unsigned int cmp, unsigned int val) { unsigned int old = *a; if (old == cmp) *a = val; return old; }
static inline unsigned int atomicAdd(unsigned int* a, unsigned int v) { unsigned int old = *a; *a = old + v; return old; }
#include "%(pre)s"
#include "%(vox)s"

struct Ref {
    std::shared_ptr<Voxelization> v;
    std::shared_ptr<Preprocess> p;
    int max_points;
};
extern "C" {
void ref_grid(const float* mn, const float* mx, const float* sz, int* out) {
    nvtype::Int3 g = VoxelizationParameter::compute_grid_size(nvtype::Float3(mx[0], mx[1], mx[2]), nvtype::Float3(mn[0], mn[1], mn[2]),
                                                             nvtype::Float3(sz[0], sz[1], sz[2]));
    out[0] = g.x; out[1] = g.y; out[2] = g.z;
}
void* ref_create(const float* mn, const float* mx, const float* sz, int max_voxels, int P, int max_points, int frames) {
    VoxelizationParameter vp;
    vp.min_range = nvtype::Float3(mn[0], mn[1], mn[2]);
    vp.max_range = nvtype::Float3(mx[0], mx[1], mx[2]);
    vp.voxel_size = nvtype::Float3(sz[0], sz[1], sz[2]);
    vp.grid_size = VoxelizationParameter::compute_grid_size(vp.max_range, vp.min_range, vp.voxel_size);
    vp.num_feature = 5;
    vp.max_voxels = max_voxels;
    vp.max_points_per_voxel = P;
    vp.max_points = max_points;
    PreprocessParameter pp;
    pp.max_points = max_points;
    pp.num_feature = 5;
    pp.max_frame_num = frames;
    Ref* r = new Ref();
    r->v = create_voxelization(vp);
    r->p = create_preprocess(pp);
    r->max_points = max_points;
    return r;
}
void ref_destroy(void* h) { delete (Ref*)h; }
int ref_forward(void* h, const float* points, int n, const float* motion, int realtime, int order) {
    Ref* r = (Ref*)h;
    int num_points = std::min(n, r->max_points);
    r->p->forward(points, num_points, motion, realtime != 0, nullptr);
    r->v->forward(r->p->get_points(), r->p->get_points_num(), (CoordinateOrder)order, nullptr);
    return r->v->num_voxels();
}
int ref_total(void* h) { return ((Ref*)h)->p->get_points_num(); }
void ref_window(void* h, float* out) { Ref* r = (Ref*)h; memcpy(out, r->p->get_points(), (size_t)r->p->get_points_num() * 5 * sizeof(float)); }
void ref_counts(void* h, int* out) {
    PreprocessImplement* p = static_cast<PreprocessImplement*>(((Ref*)h)->p.get());
    for (size_t i = 0; i < p->points_num_.size(); i++) out[i] = p->points_num_[i];
}
unsigned int ref_real(void* h) { return *static_cast<VoxelizationImplement*>(((Ref*)h)->v.get())->h_real_num_voxels_; }
void ref_output(void* h, uint16_t* feat, int* idx, unsigned int* cnt) {
    VoxelizationImplement* v = static_cast<VoxelizationImplement*>(((Ref*)h)->v.get());
    const size_t nv = (size_t)v->num_voxels();
    memcpy(feat, v->d_voxel_features_, nv * 5 * sizeof(uint16_t));
    memcpy(idx, v->d_voxel_indices_, nv * 4 * sizeof(int));
    memcpy(cnt, v->d_voxel_num_, nv * sizeof(unsigned int));
}
}
"""


def build(reference, td):
    d = os.path.join(reference, "sensor_driver", "inference", "voxelize")
    pre, vox = os.path.join(d, "preprocess_kernel.cu"), os.path.join(d, "voxelization_kernel.cu")
    for f in (pre, vox):
        if not os.path.exists(f):
            sys.exit(f"{f} is missing")
    open(os.path.join(td, "cuda_fp16.h"), "w").close()  # the one system header the two files ask for
    shim, lib = os.path.join(td, "ref.cpp"), os.path.join(td, "ref.so")
    with open(shim, "w") as f:
        f.write(SHIM % dict(pre=pre, vox=vox))
    subprocess.check_call([CXX, "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared", "-w", "-I", td, "-I", d, shim, "-o", lib])
    L = C.CDLL(lib)
    L.ref_create.restype = C.c_void_p
    L.ref_real.restype = C.c_uint
    return L


def fp(a):
    return a.ctypes.data_as(C.c_void_p)


def ref_grid(L, p):
    g = np.zeros(3, np.int32)
    L.ref_grid(fp(p["min"]), fp(p["max"]), fp(p["size"]), fp(g))
    return g


def run_reference(L, case):
    p, calls = case
    h = C.c_void_p(L.ref_create(fp(p["min"]), fp(p["max"]), fp(p["size"]), int(p["max_voxels"]), int(p["P"]), int(p["max_points"]), int(p["frames"])))
    out = []
    for rows, motion, realtime in calls:
        rows, motion = np.ascontiguousarray(rows, F), np.ascontiguousarray(motion, F)
        nv = L.ref_forward(h, fp(rows), len(rows), fp(motion), int(bool(realtime)), int(p["order"]))
        total = L.ref_total(h)
        win, cnts = np.zeros((total, 5), F), np.zeros(p["frames"], np.int32)
        L.ref_window(h, fp(win))
        L.ref_counts(h, fp(cnts))
        feat, idx, cnt = np.zeros((nv, 5), np.uint16), np.zeros((nv, 4), np.int32), np.zeros(nv, np.uint32)
        if nv:
            L.ref_output(h, fp(feat), fp(idx), fp(cnt))
        out.append(dict(window=win, window_counts=cnts, features=feat, indices=idx, counts=cnt, num=np.int64(nv), real=np.int64(L.ref_real(h))))
    L.ref_destroy(h)
    return out


def both_tests_agree(win, p):
    """no row is non-finite in x y z, and none passes the grid test while failing the range test"""
    xyz = win[:, :3]
    if not np.isfinite(xyz).all():
        return False
    g = np.asarray(vc.grid_size(p["min"], p["max"], p["size"]))
    f = np.floor((xyz - p["min"]) / p["size"])
    in_grid = ((f >= 0) & (f < g)).all(1)
    in_range = ((xyz >= p["min"]) & (xyz < p["max"])).all(1)
    return not (in_grid & ~in_range).any()


def record(L, cases, strict):
    g = {}
    for name, case in cases.items():
        p, calls = case
        ref, mine = run_reference(L, case), vc.run_case(case)
        g[f"{name}/params_f"] = np.concatenate([p["min"], p["max"], p["size"]]).astype(F)
        g[f"{name}/params_i"] = np.asarray([p["max_voxels"], p["P"], p["max_points"], p["frames"], p["order"]], np.int64)
        g[f"{name}/grid"] = ref_grid(L, p)
        g[f"{name}/calls"] = np.int64(len(calls))
        for k, ((rows, motion, realtime), r, m) in enumerate(zip(calls, ref, mine)):
            g[f"{name}/{k}/motion"], g[f"{name}/{k}/realtime"] = np.asarray(motion, F), np.int64(bool(realtime))
            if len(calls) == 1 and not name.endswith("_rev"):  # (a window's front rows are the sweep; a _rev case is its partner reversed)
                g[f"{name}/{k}/in"] = np.asarray(rows, F)
            for w in vc.WHAT:
                g[f"{name}/{k}/{w}"] = r[w]
            if len(calls) > 1 and (name not in LAST_WINDOW_ONLY or k == len(calls) - 1):
                g[f"{name}/{k}/window"] = r["window"]
            if strict:
                assert both_tests_agree(r["window"], p), f"{name} call {k}: a non-finite point or a grid-only point outside the deviation file"
                bad = vc.check_call(m, r)
                assert not bad, f"{name} call {k}: the restatement differs from the reference in {bad}"
        print(f"{name}: {[int(r['num']) for r in ref]} voxels of {[int(r['real']) for r in ref]}, window {[len(r['window']) for r in ref]}")
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as td:
        L = build(a.reference, td)
        g = record(L, vc.CASES, True)
        assert list(ref_grid(L, vc.params(mn=(0, 0, -2), mx=(1, 1, 4), size=(1, 1, 0.15)))) == [1, 1, 40]
        np.savez_compressed(vc.GOLDEN, **g)
        d = record(L, vc.DEVIATIONS, False)
        np.savez_compressed(vc.GOLDEN_DEV, **d)
    for f in (vc.GOLDEN, vc.GOLDEN_DEV):
        print(f"{f}: {os.path.getsize(f)} bytes")


if __name__ == "__main__":
    main()
