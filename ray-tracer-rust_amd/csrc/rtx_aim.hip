// rtx_aim.hip — the primary rays' stream for another eye, made on the device, for gfx950.
//
//   rtx_render_view_rows   the render pipeline (probe_kernel, order_tiles_kernel, shade_tiles_kernel) with a view's camera:
//                          its primary rays walk the tree with the child nearer the view's eye first
//
// Input: the shadow stream as uploaded (NodeDev word order, pre-order, inner.info = second child, link = the record
// behind the subtree, planes moved out by cull_delta).  Output: the same tree, the same records, below `root` the child
// whose box centre is nearer the eye first — scene_prep.cpp's stream_nearest_first, record for record.
//
// A record's new position is root + the sum, over its path to the root, of 1 + the size of the sibling visited ahead of
// it.  Pass 1 (one work-item per record): an inner node decides its children's order and writes for each child its parent
// and that size.  Pass 2 (one work-item per record): walks the path up — at most 65 steps, TreeBuilder's depth cap plus
// the root in front of the global triangles — and writes the record at its new position.  The kernel boundary is the
// visibility between the passes: no atomics, no LDS, every output record written by exactly one work-item.
//
// The kernels live in namespace rtxa: librtx.so's rtx::, rtxq::, rtxs:: and rtxv:: kernel sets stay what they were.
#include "rtx_aim.h"

namespace rtxa {

using rtx::kLeafFlag;
using rtx::NodeDev;

constexpr uint32_t kAimBlock = 256u;
constexpr uint32_t kNoParent = 0xFFFFFFFFu;
constexpr uint32_t kMaxPath = 128u;          // well above the 65 a built tree can have: a malformed stream ends the walk

struct Eye { float x, y, z; };

__device__ __forceinline__ NodeDev load_node(const NodeDev *__restrict__ nodes, uint32_t i)
{
    const uint4 *p = reinterpret_cast<const uint4 *>(nodes + i);      // 32-byte records in a hipMalloc'ed buffer
    const uint4 a = p[0], b = p[1];
    NodeDev n;
    n.lox = __uint_as_float(a.x); n.loy = __uint_as_float(a.y); n.hix = __uint_as_float(a.z); n.hiy = __uint_as_float(a.w);
    n.loz = __uint_as_float(b.x); n.hiz = __uint_as_float(b.y); n.link = b.z; n.info = b.w;
    return n;
}

// dist2 of stream_nearest_first: c_k = (0.5 lo_k + 0.5 hi_k) - eye_k, d2 = ((0 + c_0^2) + c_1^2) + c_2^2, every operation
// rounded once (no v_fma_f64 may stand in for a multiply and an add: the host's expression has none)
__device__ __forceinline__ double centre_dist2(const NodeDev &n, const Eye &e)
{
    const double c0 = __dadd_rn(__dadd_rn(__dmul_rn(0.5, (double)n.lox), __dmul_rn(0.5, (double)n.hix)), -(double)e.x);
    const double c1 = __dadd_rn(__dadd_rn(__dmul_rn(0.5, (double)n.loy), __dmul_rn(0.5, (double)n.hiy)), -(double)e.y);
    const double c2 = __dadd_rn(__dadd_rn(__dmul_rn(0.5, (double)n.loz), __dmul_rn(0.5, (double)n.hiz)), -(double)e.z);
    double d2 = __dadd_rn(0.0, __dmul_rn(c0, c0));
    d2 = __dadd_rn(d2, __dmul_rn(c1, c1));
    d2 = __dadd_rn(d2, __dmul_rn(c2, c2));
    return d2;
}

__device__ __forceinline__ uint32_t subtree_size(const NodeDev &n, uint32_t index)
{
    return (n.info & kLeafFlag) ? 1u : n.link - index;
}

// pass 1: record i >= root, when it is an inner node, orders its children a = i + 1 and b = info(i)
__global__ void __launch_bounds__(kAimBlock) aim_order_kernel(const NodeDev *__restrict__ nodes, uint32_t n_nodes, uint32_t root,
                                                              Eye eye, AimLink *__restrict__ links)
{
    const uint32_t i = root + blockIdx.x * kAimBlock + threadIdx.x;
    if (i >= n_nodes) return;
    if (i == root) links[root] = AimLink{kNoParent, 0u};
    const uint32_t info = nodes[i].info;
    if (info & kLeafFlag) return;
    const uint32_t a = i + 1u, b = info;
    if (b <= a || b >= n_nodes) return;      // (not a stream prepare_scene makes: its children keep what the buffer holds)
    const NodeDev na = load_node(nodes, a), nb = load_node(nodes, b);
    const bool a_first = !(centre_dist2(nb, eye) < centre_dist2(na, eye));
    links[a] = AimLink{i, a_first ? 0u : subtree_size(nb, b)};
    links[b] = AimLink{i, a_first ? subtree_size(na, a) : 0u};
}

// pass 2: record i goes to its new position; records before root are copied
__global__ void __launch_bounds__(kAimBlock) aim_place_kernel(const NodeDev *__restrict__ nodes, uint32_t n_nodes, uint32_t root,
                                                              const AimLink *__restrict__ links, NodeDev *__restrict__ out)
{
    const uint32_t i = blockIdx.x * kAimBlock + threadIdx.x;
    if (i >= n_nodes) return;
    NodeDev n = load_node(nodes, i);
    uint32_t pos = i;
    if (i >= root) {
        pos = root;
        uint32_t j = i;
        for (uint32_t step = 0; j != root && step < kMaxPath; ++step) {
            if (j < root || j >= n_nodes) return;
            const AimLink l = links[j];
            pos += 1u + l.before;
            j = l.parent;
        }
        if (j != root || pos >= n_nodes) return;
        if (!(n.info & kLeafFlag)) {
            const uint32_t a = i + 1u, b = n.info, size = n.link - i;
            if (b <= a || b >= n_nodes) return;
            const uint32_t second = links[a].before == 0u ? b : a;       // its `before` is the size of the child visited first
            n.link = pos + size;
            n.info = pos + 1u + links[second].before;
        }
    }
    uint4 *p = reinterpret_cast<uint4 *>(out + pos);
    p[0] = make_uint4(__float_as_uint(n.lox), __float_as_uint(n.loy), __float_as_uint(n.hix), __float_as_uint(n.hiy));
    p[1] = make_uint4(__float_as_uint(n.loz), __float_as_uint(n.hiz), n.link, n.info);
}

hipError_t launch_aim(const NodeDev *nodes, uint32_t n_nodes, uint32_t root, const float eye[3], AimLink *links, NodeDev *out,
                      hipStream_t stream)
{
    if (n_nodes == 0u) return hipSuccess;
    if (!nodes || !links || !out || root >= n_nodes) return hipErrorInvalidValue;
    const Eye e{eye[0], eye[1], eye[2]};
    const uint32_t below = n_nodes - root;
    hipLaunchKernelGGL(aim_order_kernel, dim3((below + kAimBlock - 1u) / kAimBlock), dim3(kAimBlock), 0, stream, nodes, n_nodes, root, e,
                       links);
    hipLaunchKernelGGL(aim_place_kernel, dim3((n_nodes + kAimBlock - 1u) / kAimBlock), dim3(kAimBlock), 0, stream, nodes, n_nodes, root,
                       static_cast<const AimLink *>(links), out);
    return hipGetLastError();
}

}  // namespace rtxa
