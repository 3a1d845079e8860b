// rtx_tour.hip — the walk of any area light, made on the device, for gfx950.
//
//   rtx_render_view_rows_lit    the render pipeline's kernels with another light's points, tour, boxes, margin and count
//
// rtx_scene_create makes, beside the light points, the order the shading pass walks them in (PreparedScene::light_tour: a
// nearest-neighbour tour of every batch of kMaxLightBatch samples, improved by 2-opt) and their bounding box per primary
// ray (light_boxes: one end of a tile's shaft).  For a light given per call both are made here, from the points
// rtxl::light_points_kernel has just written on the same stream.
//
// tour_kernel: one workgroup of ONE wavefront per (primary ray, batch).  The scan it reproduces is serial
// (scene_prep.cpp: light_tour_order_f32), but each of its steps is a choice among up to 127 candidates that do not depend
// on each other:
//   nearest neighbour   the unused point with the least distance, the lowest index on ties: a wave-wide minimum of
//                       (distance bits, index) — distances are >= +0, so their bits order as the values do
//   2-opt, fixed i      the serial scan takes the LOWEST j whose reversal improves, reverses, and goes on from j + 1 with
//                       the new order: the lanes evaluate the remaining j against the current order, a ballot picks the
//                       lowest improving one, the lanes reverse [i, j] together
// The batch's points, its order and the distances of all pairs (the lower triangle: 128 * 127 / 2 floats) live in LDS; a
// distance is rtx::tour_distance, the text the host compiles, so kept or recomputed it is the same bits.  `before` and
// `after` are f32 sums of two distances in the host's order (-ffp-contract=off: one rounding each).  Every loop is
// bounded whatever the points hold: 32 passes, i ascending, j strictly ascending; a NaN never compares less.
//
// No atomics, no scratch; every output word is written by exactly one work-item.
#include "rtx_tour.h"

namespace rtxt {

constexpr uint32_t kWave = 64u;
constexpr uint32_t kBatch = rtx::kMaxLightBatch;
constexpr uint32_t kPairs = kBatch * (kBatch - 1u) / 2u;
constexpr uint32_t kPasses = 32u;
static_assert(kBatch >= 1u && kBatch <= 2u * kWave, "a lane holds the nearest-neighbour state of two points");
static_assert((kPairs + 4u * kBatch) * sizeof(float) <= 65536u, "points, order and pair distances in static LDS");

// place of D(a, b), a != b, in the lower triangle
__device__ inline uint32_t pair_at(uint32_t a, uint32_t b)
{
    const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
    return hi * (hi - 1u) / 2u + lo;
}

__device__ inline unsigned long long wave_min(unsigned long long x)
{
    for (int m = 1; m < static_cast<int>(kWave); m <<= 1) {
        const unsigned long long y = __shfl_xor(x, m, static_cast<int>(kWave));
        x = y < x ? y : x;
    }
    return x;
}

__global__ void __launch_bounds__(kWave) tour_kernel(const float *__restrict__ points, uint32_t nb_light, uint32_t n_batches,
                                                     float *__restrict__ tour)
{
    __shared__ float l_point[3u * kBatch];
    __shared__ float l_dist[kPairs ? kPairs : 1u];
    __shared__ uint32_t l_order[kBatch];
    const uint32_t lane = threadIdx.x;
    const uint32_t r = blockIdx.x / n_batches, b0 = (blockIdx.x - r * n_batches) * kBatch;
    const uint32_t n = nb_light - b0 < kBatch ? nb_light - b0 : kBatch;
    const size_t first = static_cast<size_t>(r) * nb_light + b0;
    for (uint32_t k = lane; k < 3u * n; k += kWave) l_point[k] = points[3u * first + k];
    if (lane == 0u) l_order[0] = 0u;
    __syncthreads();
    for (uint32_t hi = 1u; hi < n; ++hi)
        for (uint32_t lo = lane; lo < hi; lo += kWave) l_dist[hi * (hi - 1u) / 2u + lo] = rtx::tour_distance(l_point + 3u * hi, l_point + 3u * lo);
    __syncthreads();

    // nearest neighbour from point 0: lane l answers for points l and l + 64
    bool used0 = lane == 0u, used1 = false;
    uint32_t at = 0u;
    for (uint32_t k = 1u; k < n; ++k) {
        unsigned long long key = ~0ull;
        if (lane < n && !used0) {
            const float d = l_dist[pair_at(at, lane)];
            key = (static_cast<unsigned long long>(d < __builtin_inff() ? __float_as_uint(d) : 0x7F800000u) << 32) | lane;
        }
        if (lane + kWave < n && !used1) {
            const float d = l_dist[pair_at(at, lane + kWave)];
            const unsigned long long key1 =
                (static_cast<unsigned long long>(d < __builtin_inff() ? __float_as_uint(d) : 0x7F800000u) << 32) | (lane + kWave);
            key = key1 < key ? key1 : key;
        }
        at = static_cast<uint32_t>(wave_min(key)) & (2u * kWave - 1u);     // (some point is unused: k < n)
        used0 = used0 || at == lane;
        used1 = used1 || at == lane + kWave;
        if (lane == 0u) l_order[k] = at;
    }
    __syncthreads();

    // 2-opt on the open path, position 0 fixed
    for (uint32_t pass = 0u; pass < kPasses; ++pass) {
        bool improved = false;
        for (uint32_t i = 1u; i + 1u < n; ++i) {
            uint32_t from = i + 1u;
            while (from < n) {
                const uint32_t a = l_order[i - 1u], b = l_order[i];
                const float d_ab = l_dist[pair_at(a, b)];
                uint32_t found = n;
                for (uint32_t base = from; base < n; base += kWave) {
                    const uint32_t j = base + lane;
                    bool better = false;
                    if (j < n) {
                        const uint32_t c = l_order[j];
                        float before = d_ab, after = l_dist[pair_at(a, c)];
                        if (j + 1u < n) {
                            const uint32_t e = l_order[j + 1u];
                            before = before + l_dist[pair_at(c, e)];
                            after = after + l_dist[pair_at(b, e)];
                        }
                        better = after < before;
                    }
                    const unsigned long long mask = __ballot(better);
                    if (mask != 0ull) {
                        found = base + static_cast<uint32_t>(__builtin_ctzll(mask));
                        break;
                    }
                }
                if (found >= n) break;
                if (lane < (found - i + 1u) / 2u) {                  // reverse positions [i, found]: at most 63 swaps
                    const uint32_t x = i + lane, y = found - lane;
                    const uint32_t ox = l_order[x], oy = l_order[y];
                    l_order[x] = oy;
                    l_order[y] = ox;
                }
                __syncthreads();
                improved = true;
                from = found + 1u;
            }
        }
        if (!improved) break;
    }

    for (uint32_t k = lane; k < n; k += kWave) {
        const uint32_t o = l_order[k];
        reinterpret_cast<float4 *>(tour)[first + k] = make_float4(l_point[3u * o], l_point[3u * o + 1u], l_point[3u * o + 2u], __uint_as_float(o));
    }
}

// one wavefront per primary ray
__global__ void __launch_bounds__(kWave) light_boxes_kernel(const float *__restrict__ points, uint32_t nb_light, float *__restrict__ boxes)
{
    const uint32_t lane = threadIdx.x, r = blockIdx.x;
    const float *p = points + 3u * static_cast<size_t>(r) * nb_light;
    float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
    float hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    for (uint32_t i = lane; i < nb_light; i += kWave)
        for (int k = 0; k < 3; ++k) {
            lo[k] = fminf(lo[k], p[3u * i + k]);
            hi[k] = fmaxf(hi[k], p[3u * i + k]);
        }
    for (int m = 1; m < static_cast<int>(kWave); m <<= 1)
        for (int k = 0; k < 3; ++k) {
            lo[k] = fminf(lo[k], __shfl_xor(lo[k], m, static_cast<int>(kWave)));
            hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], m, static_cast<int>(kWave)));
        }
    if (lane < 3u) boxes[6u * static_cast<size_t>(r) + lane] = lane == 0u ? lo[0] : lane == 1u ? lo[1] : lo[2];
    else if (lane < 6u) boxes[6u * static_cast<size_t>(r) + lane] = lane == 3u ? hi[0] : lane == 4u ? hi[1] : hi[2];
}

namespace {

// 0: nothing to make; else the point count, or hipErrorInvalidValue through *err
bool walk_args(const void *points, const void *out, uint32_t nb_ray, uint32_t nb_light, hipError_t *err)
{
    *err = hipSuccess;
    const uint64_t n_points = static_cast<uint64_t>(nb_ray) * nb_light;
    if (n_points == 0u) return false;
    if (!points || !out || n_points > rtx::kMaxCallLightPoints) {
        *err = hipErrorInvalidValue;
        return false;
    }
    return true;
}

}  // namespace

hipError_t launch_tour(const float *points, uint32_t nb_ray, uint32_t nb_light, float *tour, hipStream_t stream)
{
    hipError_t err;
    if (!walk_args(points, tour, nb_ray, nb_light, &err)) return err;
    if (reinterpret_cast<uintptr_t>(tour) & 15u) return hipErrorInvalidValue;
    const uint32_t n_batches = (nb_light + kBatch - 1u) / kBatch;      // nb_ray * n_batches <= 2^20
    hipLaunchKernelGGL(tour_kernel, dim3(nb_ray * n_batches), dim3(kWave), 0, stream, points, nb_light, n_batches, tour);
    return hipGetLastError();
}

hipError_t launch_light_boxes(const float *points, uint32_t nb_ray, uint32_t nb_light, float *boxes, hipStream_t stream)
{
    hipError_t err;
    if (!walk_args(points, boxes, nb_ray, nb_light, &err)) return err;
    hipLaunchKernelGGL(light_boxes_kernel, dim3(nb_ray), dim3(kWave), 0, stream, points, nb_light, boxes);
    return hipGetLastError();
}

}  // namespace rtxt
