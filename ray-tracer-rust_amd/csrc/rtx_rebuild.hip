// rtx_rebuild.hip — the sorted records of a pose whose tree is rebuilt, made on the device, for gfx950.
//
//   rtx_scene_pose_rebuilt / rtx_scene_pose_rebuilt_device    keys, the permutation, the primitive and shading records
//
// The rebuilt tree's shape is a closed form of the scene's counts (scene_prep.h: RebuildTables), so nothing is built here:
// key_kernel states every record's key from its posed own box (rebuild_key_statement, the text the host compiles too),
// a rocprim radix sort orders the (key, source position) pairs — stable, so equal keys keep uploaded order — and
// records_kernel restates every triangle at its sorted position (triangle_statement).  The boxes are the refit kernels'
// fold over those records (rtx_pose.hip), launched behind these.
//
// Both kernels are one record per work-item and memory-bound.  A 64-byte record is read and written as four 16-byte words
// (the records lie on 64-byte boundaries of the library's allocations).  No arrival counters, no spinning, no atomics; every
// output word is written by exactly one work-item, and no work-item reads what another wrote in the same launch.
//
// The kernels live in namespace rtxb: librtx.so's other kernel sets stay what they were.
#include <cstdlib>
#include <type_traits>
// librtx.so imports no getenv (tests/test_host_prep.py): rocprim's host side asks for one tuning override through
// std::getenv; inside this translation unit that expression reads a null char *, "not set", as in rtx_query.hip.
#define getenv(name) add_pointer_t<char>(nullptr)
#include <rocprim/device/device_radix_sort.hpp>
#undef getenv

#include "rtx_rebuild.h"

namespace rtxb {

// The one instantiation of the 64-bit sort, for the size query and the sort alike: n (key, source position) pairs by rising
// key, all 64 bits, stable.  A source position is a type of its own, so that every kernel of this sort — the copies of the
// values too — differs in name from the 32-bit sort's of rtx_query.hip (the regrouping pass): that unit and its code
// object stay what they were, and no rocprim kernel is in the library twice.
struct SourcePosition {
    uint32_t at;
};
static_assert(sizeof(SourcePosition) == sizeof(uint32_t) && alignof(SourcePosition) == alignof(uint32_t), "four bytes, as the index words");

static hipError_t sort_pairs(void *temp, size_t &temp_bytes, const uint64_t *keys, uint64_t *keys_sorted, const uint32_t *values,
                             uint32_t *values_sorted, uint32_t n_entries, hipStream_t stream)
{
    return rocprim::radix_sort_pairs(temp, temp_bytes, keys, keys_sorted, reinterpret_cast<const SourcePosition *>(values),
                                     reinterpret_cast<SourcePosition *>(values_sorted), n_entries, 0u, 64u, stream);
}

hipError_t sort_temp_bytes(uint32_t n_entries, size_t *bytes)
{
    *bytes = 0;
    return sort_pairs(nullptr, *bytes, nullptr, nullptr, nullptr, nullptr, n_entries, nullptr);
}

union RecordWords {
    rtx::TriRec rec;
    uint4 w[4];
    __device__ RecordWords() : w{} {}
};
static_assert(sizeof(RecordWords) == 64, "a primitive record is four 16-byte words");

__device__ inline void load_record(const rtx::TriRec *from, RecordWords &r)
{
    const uint4 *p = reinterpret_cast<const uint4 *>(from);
    for (int k = 0; k < 4; ++k) r.w[k] = p[k];
}

__global__ void __launch_bounds__(kRebuildBlock) key_kernel(RebuildArgs a)
{
    const uint32_t p = blockIdx.x * kRebuildBlock + threadIdx.x;
    if (p >= a.n_prims - a.n_global) return;
    const uint32_t j = a.n_global + p;
    RecordWords r;
    load_record(a.tris + j, r);
    const bool sphere = a.shade[r.rec.idx].kind != 0u;
    if (!sphere) {
        const float *v = a.pose + 9u * static_cast<size_t>(a.tri_of[r.rec.idx]);
        float x[9], e1[3], e2[3], normal[3];
        for (int k = 0; k < 9; ++k) x[k] = v[k];
        rtx::triangle_statement(x, x + 3, x + 6, e1, e2, normal, r.rec.bmin, r.rec.bmax);
    }
    a.keys[p] = rtx::rebuild_key_statement(r.rec.bmin, r.rec.bmax, sphere, a.bound, a.scale);
    a.index[p] = j;
}

__global__ void __launch_bounds__(kRebuildBlock) records_kernel(RebuildArgs a)
{
    const uint32_t j = blockIdx.x * kRebuildBlock + threadIdx.x;
    if (j >= a.n_prims) return;
    const uint32_t from = j < a.n_global ? j : a.perm[j - a.n_global];
    RecordWords r;
    load_record(a.tris + from, r);
    rtx::ShadeRec sh = a.shade[r.rec.idx];
    if (sh.kind == 0u) {
        const float *p = a.pose + 9u * static_cast<size_t>(a.tri_of[r.rec.idx]);
        float v[9];
        for (int k = 0; k < 9; ++k) v[k] = p[k];
        r.rec.v0[0] = v[0];
        r.rec.v0[1] = v[1];
        r.rec.v0[2] = v[2];
        rtx::triangle_statement(v, v + 3, v + 6, r.rec.e1, r.rec.e2, sh.normal, r.rec.bmin, r.rec.bmax);
    }
    sh.rank = a.rank ? a.rank[r.rec.idx] : r.rec.idx;
    uint4 *out = reinterpret_cast<uint4 *>(a.out_tris + j);
    for (int k = 0; k < 4; ++k) out[k] = r.w[k];
    a.out_shade[r.rec.idx] = sh;
}

hipError_t launch_rebuild(const RebuildArgs &a, hipStream_t stream)
{
    if (a.n_prims == 0u) return hipSuccess;
    if (!a.tris || !a.shade || !a.tri_of || !a.pose || !a.out_tris || !a.out_shade || a.n_global > a.n_prims)
        return hipErrorInvalidValue;
    const uint32_t n_tree = a.n_prims - a.n_global;
    if (n_tree != 0u) {
        if (!a.keys || !a.keys_sorted || !a.index || !a.perm || !a.temp) return hipErrorInvalidValue;
        hipLaunchKernelGGL(key_kernel, dim3((n_tree + kRebuildBlock - 1u) / kRebuildBlock), dim3(kRebuildBlock), 0, stream, a);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        size_t temp_bytes = a.temp_bytes;
        e = sort_pairs(a.temp, temp_bytes, a.keys, a.keys_sorted, a.index, a.perm, n_tree, stream);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(records_kernel, dim3((a.n_prims + kRebuildBlock - 1u) / kRebuildBlock), dim3(kRebuildBlock), 0, stream, a);
    return hipGetLastError();
}

}  // namespace rtxb
