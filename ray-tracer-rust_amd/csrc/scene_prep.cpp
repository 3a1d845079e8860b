// scene_prep.cpp — host-side scene preparation (see scene_prep.h).
//
// Float arithmetic that feeds pixel values (camera basis, e1/e2/normal, light points)
// follows the reference's operation order, one IEEE binary32 rounding per operation;
// build with -ffp-contract=off.  Reference citations are path:line under the reference
// repository (antoinedesbois/Ray-Tracer-Rust).
#include "scene_prep.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <numeric>

namespace rtx {

namespace {

struct V3 { float x, y, z; };

inline V3 load3(const float *p) { return V3{p[0], p[1], p[2]}; }
inline void store3(float *p, V3 a) { p[0] = a.x; p[1] = a.y; p[2] = a.z; }
inline V3 operator-(V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }

// nalgebra 0.11 dot: accumulator starts at zero, terms added in x, y, z order
inline float dot3(V3 a, V3 b)
{
    float acc = 0.0f;
    acc = acc + a.x * b.x;
    acc = acc + a.y * b.y;
    acc = acc + a.z * b.z;
    return acc;
}
inline V3 cross3(V3 a, V3 b)
{
    return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
// Unit::new_normalize: divide each component by sqrt(dot(v,v))
inline V3 unit3(V3 a)
{
    const float n = std::sqrt(dot3(a, a));
    return V3{a.x / n, a.y / n, a.z / n};
}

inline float lesser(float a, float b) { return a < b ? a : b; }    // min_float, triangle.rs:37-39
inline float greater(float a, float b) { return a < b ? b : a; }   // max_float, triangle.rs:41-43

}  // namespace

// Camera::new — src/tracer/utils/camera.rs:17-35
void camera_new(const float eye[3], const float look_at[3], const float up[3],
                float u[3], float v[3], float w[3])
{
    const V3 ww = unit3(load3(eye) - load3(look_at));
    const V3 o = unit3(load3(up));
    const V3 uu = unit3(cross3(o, ww));
    const V3 vv = unit3(cross3(uu, ww));
    store3(u, uu);
    store3(v, vv);
    store3(w, ww);
}

// Triangle::new + get_bounding_box — src/tracer/primitives/triangle.rs:22-34, :45-56
void triangle_derive(const float v0[3], const float v1[3], const float v2[3],
                     float e1[3], float e2[3], float normal[3], float bmin[3], float bmax[3])
{
    triangle_statement(v0, v1, v2, e1, e2, normal, bmin, bmax);   // scene_prep.h: the statement the device compiles too
}

// Triangle::get_sample — triangle.rs:113-127: scene_prep.h's light_sample_point, the statement the device compiles too
void light_sample(const float v0[3], const float v1[3], const float v2[3], float u, float v, float out[3])
{
    light_sample_point(v0, v1, v2, u, v, out);
}

// light points: for ray r of a pixel and sample i the reference reads T[(r*NB_RAY + i) % len] (src/main.rs:194-196) —
// the same points for every pixel
void light_points_of(const float tri[9], const SampleSource &samples, uint32_t nb_ray, uint32_t nb_light, float *out)
{
    for (uint32_t r = 0; r < nb_ray; ++r)
        for (uint32_t i = 0; i < nb_light; ++i) {
            const size_t k = (static_cast<size_t>(r) * nb_ray + i) % samples.n;
            float u, v;
            samples.pair(k, &u, &v);
            light_sample_point(tri, tri + 3, tri + 6, u, v, &out[3 * (static_cast<size_t>(r) * nb_light + i)]);
        }
}

// Color::to_rgba on one channel — src/tracer/utils/color.rs:10-13,28-33.
// Rust's `as u8` truncates toward zero, saturates, and maps NaN to 0.
uint8_t gamma_quantise(float linear)
{
    const float gamma = 2.2f;
    const float enc = std::pow(linear, 1.0f / gamma) * 255.0f;
    if (std::isnan(enc) || enc <= 0.0f) return 0;
    if (enc >= 255.0f) return 255;
    return static_cast<uint8_t>(enc);
}

// The kernel never evaluates powf: the byte of a channel is a step function of the f32
// input, so the 255 step positions are located here with the host libm (the same powf
// the reference's f32::powf resolves to) and the kernel counts thresholds <= x.
// thr[b] (b >= 1) = smallest non-negative float x with gamma_quantise(x) >= b.
int build_gamma_thresholds(float thr[256])
{
    auto as_float = [](uint32_t bits) { float f; std::memcpy(&f, &bits, 4); return f; };
    const uint32_t hi_bits = 0x40000000u;  // 2.0f: quantises to 255
    if (gamma_quantise(as_float(hi_bits)) != 255 || gamma_quantise(0.0f) != 0) return RTX_ERR_INTERNAL;
    thr[0] = -std::numeric_limits<float>::infinity();
    for (int b = 1; b < 256; ++b) {
        uint32_t lo = 0, hi = hi_bits;   // q(lo) < b <= q(hi); positive floats order like their bit patterns
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (gamma_quantise(as_float(mid)) >= b) hi = mid; else lo = mid;
        }
        // the bisection assumed a clean step; verify it on the neighbourhood
        for (uint32_t k = 1; k <= 256; ++k) {
            if (hi >= k && gamma_quantise(as_float(hi - k)) >= b) return RTX_ERR_INTERNAL;
            if (gamma_quantise(as_float(hi + k - 1)) < b) return RTX_ERR_INTERNAL;
        }
        thr[b] = as_float(hi);
    }
    for (int b = 2; b < 256; ++b)
        if (!(thr[b] >= thr[b - 1])) return RTX_ERR_INTERNAL;
    return RTX_OK;
}

// The reference's own tree — BoundingVolumeHierarchy::new, bounding_volume_hierarchy.rs:173-226.
// Clusters by bbox *extent* because get_center() returns max-min (bounding_box.rs:183-189); O(n^2)
// per level like the original.  Two things need it:
//   - the left-to-right leaf order decides which of two exactly-equidistant triangles the reference
//     returns (the right-most leaf, :123-130)  -> out_rank;
//   - for rays with a zero direction component the reference's result depends on the tree itself (a
//     -0.0 component makes an ancestor's slab test reject through +-inf while a flat leaf accepts
//     through ignored NaNs), so those rays are traced against THIS tree -> out_stream: pre-order,
//     skip-linked NodeRecs, one triangle per leaf, leaf info = kLeafFlag | caller index.
void stream_nearest_first(const std::vector<NodeRec> &nodes, uint32_t root, const float *point, std::vector<NodeRec> &out)
{
    out.clear();
    out.reserve(nodes.size());
    for (uint32_t i = 0; i < root && i < nodes.size(); ++i) out.push_back(nodes[i]);
    if (root >= nodes.size()) return;
    auto dist2 = [&](const NodeRec &n) {
        double d2 = 0;
        for (int k = 0; k < 3; ++k) {
            const double c = 0.5 * double(n.bmin[k]) + 0.5 * double(n.bmax[k]) - double(point[k]);
            d2 += c * c;
        }
        return d2;
    };
    struct Item { uint32_t node; uint32_t close; };       // close != kNone: the subtree of out[close] ends here
    constexpr uint32_t none = 0xFFFFFFFFu;
    std::vector<Item> todo;
    todo.push_back({root, none});
    while (!todo.empty()) {
        const Item it = todo.back();
        todo.pop_back();
        if (it.close != none) { out[it.close].link = static_cast<uint32_t>(out.size()); continue; }
        const NodeRec &n = nodes[it.node];
        const uint32_t pos = static_cast<uint32_t>(out.size());
        out.push_back(n);
        if (n.info & kLeafFlag) continue;
        const uint32_t a = it.node + 1u, b = n.info;      // first child: the next record; second: named by info
        const bool a_first = !(dist2(nodes[b]) < dist2(nodes[a]));
        todo.push_back({0u, pos});
        todo.push_back({a_first ? b : a, none});
        todo.push_back({a_first ? a : b, none});
    }
    // a root in front of the tree proper (the global triangles' leaf beside it) spans the whole stream
    if (root != 0u && !(out[0].info & kLeafFlag)) out[0].link = static_cast<uint32_t>(out.size());
    for (size_t i = root; i < out.size(); ++i)             // inner nodes name their second child, as in `nodes`
        if (!(out[i].info & kLeafFlag)) {
            const NodeRec &first = out[i + 1];
            out[i].info = (first.info & kLeafFlag) ? static_cast<uint32_t>(i) + 2u : first.link;
        }
}

int ref_tree_build(uint32_t n, const float *v0v1v2, uint32_t *out_rank, std::vector<NodeRec> *out_stream)
{
    if (!n || !v0v1v2) return RTX_ERR_BAD_ARG;
    std::vector<float> boxes(6 * static_cast<size_t>(n));
    for (uint32_t i = 0; i < n; ++i) {
        const float *t = v0v1v2 + 9 * static_cast<size_t>(i);
        for (int k = 0; k < 3; ++k) {                     // Triangle::get_bounding_box, triangle.rs:45-56
            boxes[6 * static_cast<size_t>(i) + k] = lesser(lesser(t[k], t[3 + k]), t[6 + k]);
            boxes[6 * static_cast<size_t>(i) + 3 + k] = greater(greater(t[k], t[3 + k]), t[6 + k]);
        }
    }
    return ref_tree_build_boxes(n, boxes.data(), out_rank, out_stream);
}

int ref_tree_build_boxes(uint32_t n, const float *lo_hi, uint32_t *out_rank, std::vector<NodeRec> *out_stream)
{
    if (!n || !lo_hi) return RTX_ERR_BAD_ARG;
    struct Cluster { float lo[3], hi[3]; int32_t left, right; };   // left < 0: leaf
    std::vector<Cluster> pool;
    pool.reserve(2 * static_cast<size_t>(n));
    std::vector<V3> extent;
    extent.reserve(2 * static_cast<size_t>(n));
    auto push_extent = [&](const Cluster &c) {
        extent.push_back(V3{c.hi[0] - c.lo[0], c.hi[1] - c.lo[1], c.hi[2] - c.lo[2]});
    };
    std::vector<int32_t> level(n), next;
    for (uint32_t i = 0; i < n; ++i) {
        Cluster c;
        std::memcpy(c.lo, lo_hi + 6 * static_cast<size_t>(i), 12);
        std::memcpy(c.hi, lo_hi + 6 * static_cast<size_t>(i) + 3, 12);
        c.left = -1;
        c.right = static_cast<int32_t>(i);   // leaf: right holds the primitive index
        pool.push_back(c);
        push_extent(c);
        level[i] = static_cast<int32_t>(i);
    }
    while (level.size() > 1) {
        next.clear();
        while (level.size() > 1) {
            const int32_t last = level.back();           // nodes.pop()
            level.pop_back();
            const V3 ref = extent[last];
            float best = FLT_MAX;
            size_t best_at = SIZE_MAX;
            for (size_t i = 0; i < level.size(); ++i) {
                const V3 d = ref - extent[level[i]];
                const float dist = std::sqrt(dot3(d, d));
                if (dist < best) { best = dist; best_at = i; }   // strict: first minimum wins
            }
            if (best_at == SIZE_MAX) return RTX_ERR_UNSUPPORTED;  // the reference would panic in swap_remove
            const int32_t partner = level[best_at];      // swap_remove(best_at)
            level[best_at] = level.back();
            level.pop_back();
            Cluster m;
            const Cluster &a = pool[last], &b = pool[partner];   // BVHNode::new(left = last, right = closest)
            for (int k = 0; k < 3; ++k) {                         // BoundingBox::new_from, bounding_box.rs:25-96
                m.lo[k] = a.lo[k] < b.lo[k] ? a.lo[k] : b.lo[k];
                m.hi[k] = a.hi[k] > b.hi[k] ? a.hi[k] : b.hi[k];
            }
            m.left = last;
            m.right = partner;
            next.push_back(static_cast<int32_t>(pool.size()));
            pool.push_back(m);
            push_extent(m);
        }
        if (level.size() == 1) next.push_back(level[0]);  // odd one out goes last
        level.swap(next);
    }
    // pre-order walk, left before right (the order BVHNode::intersect recurses in, :88-107)
    if (out_stream) { out_stream->clear(); out_stream->reserve(pool.size()); }
    struct Frame { int32_t id; uint32_t pos; bool done; };
    std::vector<Frame> stack{{level[0], 0u, false}};
    uint32_t rank = 0;
    while (!stack.empty()) {
        Frame f = stack.back();
        stack.pop_back();
        const Cluster &c = pool[f.id];
        if (f.done) {   // subtree finished: the skip link of this inner node is the next position
            if (out_stream) (*out_stream)[f.pos].link = static_cast<uint32_t>(out_stream->size());
            continue;
        }
        NodeRec rec;
        std::memcpy(rec.bmin, c.lo, 12);
        std::memcpy(rec.bmax, c.hi, 12);
        const uint32_t pos = out_stream ? static_cast<uint32_t>(out_stream->size()) : 0u;
        if (c.left < 0) {
            rec.info = kLeafFlag | static_cast<uint32_t>(c.right);
            rec.link = 1;
            if (out_stream) out_stream->push_back(rec);
            if (out_rank) out_rank[c.right] = rank;
            ++rank;
            continue;
        }
        rec.info = 0;
        rec.link = 0;
        if (out_stream) out_stream->push_back(rec);
        stack.push_back({f.id, pos, true});
        stack.push_back({c.right, 0u, false});
        stack.push_back({c.left, 0u, false});
    }
    return rank == n ? RTX_OK : RTX_ERR_INTERNAL;
}

int ref_leaf_rank(uint32_t n, const float *v0v1v2, uint32_t *out_rank)
{
    if (!out_rank) return RTX_ERR_BAD_ARG;
    return ref_tree_build(n, v0v1v2, out_rank, nullptr);
}

// --------------------------------------------------------------------------
// Acceleration structure for the kernel: binned-SAH BVH over the triangles' exact
// AABBs, flattened in pre-order with skip links.  Its shape is free: the reference
// visits every node whose box test passes and counts a leaf only when the leaf's own
// box passes, and IEEE subtraction/division are monotone, so a ray that passes a
// triangle's box passes every box that contains it — any tree over the same leaf
// boxes yields the same hit set (DESIGN.md "Why a different tree gives the same image").

namespace {

struct Prim {
    float lo[3], hi[3];
    float c[3];
    uint32_t idx;
    uint32_t kind;   // 0 triangle, 1 sphere
};

struct Box {
    float lo[3], hi[3];
    void reset()
    {
        for (int k = 0; k < 3; ++k) { lo[k] = FLT_MAX; hi[k] = -FLT_MAX; }
    }
    void grow(const float l[3], const float h[3])
    {
        for (int k = 0; k < 3; ++k) {
            if (l[k] < lo[k]) lo[k] = l[k];
            if (h[k] > hi[k]) hi[k] = h[k];
        }
    }
    double half_area() const
    {
        const double dx = double(hi[0]) - lo[0], dy = double(hi[1]) - lo[1], dz = double(hi[2]) - lo[2];
        return dx * dy + dy * dz + dz * dx;
    }
};

class TreeBuilder {
public:
    // depth_cap: levels the tree may have.  A range that could not be finished within the cap by halving is halved
    // from there on (median split along its widest centroid axis) instead of split by the SAH.
    TreeBuilder(std::vector<Prim> &prims, std::vector<NodeRec> &nodes, uint32_t leaf_max, double box_cost,
                uint32_t depth_cap = 64u, const float *light = nullptr)
        : prims_(prims), nodes_(nodes), leaf_max_(leaf_max), box_cost_(box_cost), depth_cap_(depth_cap), light_(light) {}

    uint32_t leaves = 0, max_leaf = 0, depth = 0;

    void build(uint32_t begin, uint32_t end, uint32_t level)
    {
        if (level + 1 > depth) depth = level + 1;
        const uint32_t count = end - begin;
        Box bounds, cbounds;
        bounds.reset();
        cbounds.reset();
        for (uint32_t i = begin; i < end; ++i) {
            bounds.grow(prims_[i].lo, prims_[i].hi);
            cbounds.grow(prims_[i].c, prims_[i].c);
        }
        const uint32_t self = static_cast<uint32_t>(nodes_.size());
        NodeRec rec;
        std::memcpy(rec.bmin, bounds.lo, 12);
        std::memcpy(rec.bmax, bounds.hi, 12);
        rec.link = 0;
        rec.info = 0;
        nodes_.push_back(rec);

        uint32_t mid = 0;
        uint32_t halvings = 0;                   // ceil(log2(count)): levels a balanced subtree over this range needs below here
        while ((1ull << halvings) < count) ++halvings;
        const bool balanced = level + 1u + halvings + 1u >= depth_cap_;
        bool split = false;
        if (balanced && count > 1) {
            int axis = 0;
            for (int k = 1; k < 3; ++k)
                if (cbounds.hi[k] - cbounds.lo[k] > cbounds.hi[axis] - cbounds.lo[axis]) axis = k;
            mid = begin + count / 2;
            std::nth_element(prims_.begin() + begin, prims_.begin() + mid, prims_.begin() + end,
                             [axis](const Prim &a, const Prim &b) { return a.c[axis] < b.c[axis]; });
            split = count > leaf_max_;
        } else {
            split = count > 1 && choose_split(begin, end, bounds, cbounds, mid);
        }
        if (!split && count > leaf_max_) {        // coincident centroids: split by position in the list
            mid = begin + count / 2;
            split = true;
        }
        if (!split) {                             // a leaf holds one arm of Primitive: split a mixed range by arm
            auto it = std::partition(prims_.begin() + begin, prims_.begin() + end, [](const Prim &p) { return p.kind == 0u; });
            mid = static_cast<uint32_t>(it - prims_.begin());
            split = mid > begin && mid < end;
        }
        if (!split) {
            nodes_[self].info = kLeafFlag | (prims_[begin].kind ? kSphereFlag : 0u) | begin;
            nodes_[self].link = count;
            ++leaves;
            if (count > max_leaf) max_leaf = count;
            return;
        }
        if (light_) mid = lightward_second(begin, mid, end);
        build(begin, mid, level + 1);
        build(mid, end, level + 1);
        nodes_[self].link = static_cast<uint32_t>(nodes_.size());
    }

    // Which child comes first in the stream is free (the walks visit every box that passes; closest hits take a minimum,
    // shadow rays any occluder).  With a light position given, the child whose primitives lie NEARER the light goes second:
    // a walk then meets the far side of every split first, which is where the shadow rays of the lit surfaces below and
    // around a mesh enter it (measured: the 1M-triangle soup -1.5 %, 3.5 % fewer box records; profiles/r03).
    uint32_t lightward_second(uint32_t begin, uint32_t mid, uint32_t end)
    {
        auto mean_dist2 = [&](uint32_t a, uint32_t b) {
            double c[3] = {0, 0, 0};
            for (uint32_t i = a; i < b; ++i)
                for (int k = 0; k < 3; ++k) c[k] += prims_[i].c[k];
            double d2 = 0;
            for (int k = 0; k < 3; ++k) { const double d = c[k] / double(b - a) - light_[k]; d2 += d * d; }
            return d2;
        };
        const bool first_is_nearer = mean_dist2(begin, mid) < mean_dist2(mid, end);
        if (!first_is_nearer) return mid;                                     // already in the wanted order
        std::rotate(prims_.begin() + begin, prims_.begin() + mid, prims_.begin() + end);
        return begin + (end - mid);
    }

private:
    static constexpr int kBins = 32;

    bool choose_split(uint32_t begin, uint32_t end, const Box &bounds, const Box &cbounds, uint32_t &mid)
    {
        const uint32_t count = end - begin;
        const double parent_area = bounds.half_area();
        double best_cost = std::numeric_limits<double>::infinity();
        int best_axis = -1, best_bin = -1;
        for (int axis = 0; axis < 3; ++axis) {
            const double lo = cbounds.lo[axis], span = double(cbounds.hi[axis]) - lo;
            if (!(span > 0)) continue;
            Box bin_box[kBins];
            uint32_t bin_n[kBins] = {0};
            for (auto &b : bin_box) b.reset();
            const double scale = kBins / span;
            for (uint32_t i = begin; i < end; ++i) {
                int b = static_cast<int>((prims_[i].c[axis] - lo) * scale);
                b = std::min(std::max(b, 0), kBins - 1);
                bin_box[b].grow(prims_[i].lo, prims_[i].hi);
                ++bin_n[b];
            }
            double right_area[kBins];
            uint32_t right_n[kBins];
            Box acc;
            acc.reset();
            uint32_t n = 0;
            for (int b = kBins - 1; b > 0; --b) {
                if (bin_n[b]) acc.grow(bin_box[b].lo, bin_box[b].hi);
                n += bin_n[b];
                right_area[b] = n ? acc.half_area() : 0.0;
                right_n[b] = n;
            }
            acc.reset();
            n = 0;
            for (int b = 0; b < kBins - 1; ++b) {
                if (bin_n[b]) acc.grow(bin_box[b].lo, bin_box[b].hi);
                n += bin_n[b];
                if (!n || !right_n[b + 1]) continue;
                const double cost = acc.half_area() * n + right_area[b + 1] * right_n[b + 1];
                if (cost < best_cost) { best_cost = cost; best_axis = axis; best_bin = b; }
            }
        }
        if (best_axis < 0) return false;
        if (count <= leaf_max_ && parent_area > 0) {
            // SAH termination: a leaf costs count triangle tests; a split costs two box tests plus
            // the children's expected triangle tests
            const double split_cost = 2.0 * box_cost_ + best_cost / parent_area;
            if (static_cast<double>(count) <= split_cost) return false;
        }
        const double lo = cbounds.lo[best_axis];
        const double scale = kBins / (double(cbounds.hi[best_axis]) - lo);
        auto it = std::partition(prims_.begin() + begin, prims_.begin() + end, [&](const Prim &p) {
            int b = static_cast<int>((p.c[best_axis] - lo) * scale);
            b = std::min(std::max(b, 0), kBins - 1);
            return b <= best_bin;
        });
        mid = static_cast<uint32_t>(it - prims_.begin());
        return mid > begin && mid < end;
    }

    std::vector<Prim> &prims_;
    std::vector<NodeRec> &nodes_;
    uint32_t leaf_max_;
    double box_cost_;
    uint32_t depth_cap_;
    const float *light_;   // NULL: children in the order the split made them; else the child nearer to *light_ second
};

}  // namespace

void light_tour_order(const float *points, uint32_t n, uint32_t *order)
{
    if (n == 0u) return;
    std::vector<double> dist(static_cast<size_t>(n) * n);
    for (uint32_t a = 0; a < n; ++a)
        for (uint32_t b = 0; b < n; ++b) {
            double q = 0.0;
            for (int k = 0; k < 3; ++k) {
                const double e = static_cast<double>(points[3 * a + k]) - static_cast<double>(points[3 * b + k]);
                q += e * e;
            }
            dist[static_cast<size_t>(a) * n + b] = std::sqrt(q);
        }
    auto D = [&](uint32_t a, uint32_t b) { return dist[static_cast<size_t>(a) * n + b]; };
    // nearest neighbour from point 0; `d < best` only: a NaN or infinite distance never wins, and a step that nothing
    // wins goes to the lowest index left
    std::vector<char> used(n, 0);
    order[0] = 0u;
    used[0] = 1;
    for (uint32_t k = 1; k < n; ++k) {
        const uint32_t at = order[k - 1u];
        uint32_t next = n;
        double best = std::numeric_limits<double>::infinity();
        for (uint32_t j = 0; j < n; ++j) {
            if (used[j]) continue;
            if (next == n) next = j;
            const double d = D(at, j);
            if (d < best) { best = d; next = j; }
        }
        order[k] = next;
        used[next] = 1;
    }
    // 2-opt on the open path: reversing positions [i, j] replaces the edges (i-1, i) and (j, j+1) by (i-1, j) and
    // (i, j+1) (the last one only when j is not the path's end); position 0 never moves
    for (uint32_t pass = 0; pass < 32u; ++pass) {
        bool improved = false;
        for (uint32_t i = 1; i + 1u < n; ++i)
            for (uint32_t j = i + 1u; j < n; ++j) {
                double before = D(order[i - 1u], order[i]), after = D(order[i - 1u], order[j]);
                if (j + 1u < n) {
                    before += D(order[j], order[j + 1u]);
                    after += D(order[i], order[j + 1u]);
                }
                if (after < before) {
                    std::reverse(order + i, order + j + 1u);
                    improved = true;
                }
            }
        if (!improved) break;
    }
}

void light_tour_order_f32(const float *points, uint32_t n, uint32_t *order)
{
    if (n == 0u) return;
    auto D = [&](uint32_t a, uint32_t b) { return tour_distance(points + 3 * a, points + 3 * b); };
    std::vector<char> used(n, 0);
    order[0] = 0u;
    used[0] = 1;
    for (uint32_t k = 1; k < n; ++k) {
        const uint32_t at = order[k - 1u];
        uint32_t next = n;
        float best = std::numeric_limits<float>::infinity();
        for (uint32_t j = 0; j < n; ++j) {
            if (used[j]) continue;
            if (next == n) next = j;
            const float d = D(at, j);
            if (d < best) { best = d; next = j; }
        }
        order[k] = next;
        used[next] = 1;
    }
    for (uint32_t pass = 0; pass < 32u; ++pass) {
        bool improved = false;
        for (uint32_t i = 1; i + 1u < n; ++i)
            for (uint32_t j = i + 1u; j < n; ++j) {
                float before = D(order[i - 1u], order[i]), after = D(order[i - 1u], order[j]);
                if (j + 1u < n) {
                    before = before + D(order[j], order[j + 1u]);
                    after = after + D(order[i], order[j + 1u]);
                }
                if (after < before) {
                    std::reverse(order + i, order + j + 1u);
                    improved = true;
                }
            }
        if (!improved) break;
    }
}

void light_boxes_of(const float *points, uint32_t nb_ray, uint32_t nb_light, float *out)
{
    for (uint32_t r = 0; r < nb_ray; ++r) {
        float *b = out + 6 * static_cast<size_t>(r);
        for (int k = 0; k < 3; ++k) { b[k] = std::numeric_limits<float>::infinity(); b[3 + k] = -b[k]; }
        for (uint32_t i = 0; i < nb_light; ++i) {
            const float *p = points + 3 * (static_cast<size_t>(r) * nb_light + i);
            for (int k = 0; k < 3; ++k) { b[k] = std::fmin(b[k], p[k]); b[3 + k] = std::fmax(b[3 + k], p[k]); }
        }
    }
}

float shaft_delta_of(float scene_magnitude, const float *light_boxes, size_t n)
{
    float magnitude = scene_magnitude;
    for (size_t k = 0; k < n; ++k)
        if (std::isfinite(light_boxes[k])) magnitude = std::fmax(magnitude, std::fabs(light_boxes[k]));
    return magnitude * 0x1p-16f + 0x1p-100f;
}

void light_walk_of(const float tri[9], const SampleSource &samples, uint32_t nb_ray, uint32_t nb_light,
                   std::vector<float> &points, std::vector<float> &tour, std::vector<uint32_t> &order_out,
                   std::vector<float> &boxes)
{
    points.resize(3 * static_cast<size_t>(nb_ray) * nb_light);
    light_points_of(tri, samples, nb_ray, nb_light, points.data());

    // the order of walking them (scene_prep.h: light_tour): per primary ray, per batch of the shading pass
    tour.resize(4 * static_cast<size_t>(nb_ray) * nb_light);
    order_out.resize(static_cast<size_t>(nb_ray) * nb_light);
    for (uint32_t r = 0; r < nb_ray; ++r)
        for (uint32_t b0 = 0; b0 < nb_light; b0 += kMaxLightBatch) {
            const uint32_t bc = std::min(nb_light - b0, kMaxLightBatch);
            const size_t first = static_cast<size_t>(r) * nb_light + b0;
            uint32_t order[kMaxLightBatch];
            light_tour_order(&points[3 * first], bc, order);
            for (uint32_t k = 0; k < bc; ++k) {
                std::memcpy(&tour[4 * (first + k)], &points[3 * (first + order[k])], 12);
                std::memcpy(&tour[4 * (first + k) + 3], &order[k], 4);
                order_out[first + k] = b0 + order[k];
            }
        }

    // bounding box of the light points of primary ray r: one end of a tile's shaft (rtx_pass_schedule.hpp: shaft_cut)
    boxes.assign(6 * static_cast<size_t>(nb_ray), 0.0f);
    light_boxes_of(points.data(), nb_ray, nb_light, boxes.data());
}

void light_walk_statement(const PreparedScene &p, const float tri[9], uint32_t count, const SampleSource &samples, uint32_t *order,
                          float *boxes, float *shaft_delta)
{
    const size_t n = static_cast<size_t>(p.nb_ray) * count;
    std::vector<float> points(3u * n), box(6u * static_cast<size_t>(p.nb_ray));
    light_points_of(tri, samples, p.nb_ray, count, points.data());
    light_boxes_of(points.data(), p.nb_ray, count, box.data());
    if (boxes) std::memcpy(boxes, box.data(), box.size() * sizeof(float));
    if (shaft_delta) *shaft_delta = shaft_delta_of(p.scene_magnitude, box.data(), box.size());
    if (!order) return;
    for (uint32_t r = 0; r < p.nb_ray; ++r)
        for (uint32_t b0 = 0; b0 < count; b0 += kMaxLightBatch) {
            const uint32_t bc = std::min(count - b0, kMaxLightBatch);
            const size_t first = static_cast<size_t>(r) * count + b0;
            light_tour_order_f32(&points[3u * first], bc, order + first);
            for (uint32_t k = 0; k < bc; ++k) order[first + k] += b0;
        }
}

int resample_scene(PreparedScene &s, const SampleSource &samples)
{
    if (!samples.n) return RTX_ERR_BAD_ARG;
    try {
        std::vector<float> points, tour, boxes, grown;
        std::vector<uint32_t> order;
        light_walk_of(s.light_v, samples, s.nb_ray, s.nb_light_sample, points, tour, order, boxes);
        const float shaft_delta = shaft_delta_of(s.scene_magnitude, boxes.data(), boxes.size());
        if (!std::isfinite(shaft_delta)) return RTX_ERR_UNSUPPORTED;
        const size_t words = 2 * static_cast<size_t>(samples.n);
        if (samples.table && s.samples.capacity() < words) grown.reserve(words);
        // Nothing below allocates: the scene changes whole or not at all.  A caller's table is copied into the scene's own
        // array where it fits, so that a table per frame neither maps nor unmaps host memory: measured, giving back a 16 MB
        // array a device has copied from stalls the process's next HIP call for milliseconds.  An
        // insert within the capacity does not reallocate.
        if (samples.table) {
            if (grown.capacity()) s.samples.swap(grown);
            s.samples.clear();
            s.samples.insert(s.samples.end(), samples.table, samples.table + words);
        } else {
            std::vector<float>().swap(s.samples);
        }
        s.light_points.swap(points);
        s.light_tour.swap(tour);
        s.light_order.swap(order);
        s.light_boxes.swap(boxes);
        s.shaft_delta = shaft_delta;
        s.n_samples = samples.n;
        s.seeded = samples.table == nullptr;
        s.sample_seed = s.seeded ? samples.seed : 0;
        ++s.table_generation;
    } catch (...) {
        return RTX_ERR_OOM;
    }
    return RTX_OK;
}

int prepare_scene(const RtxSceneDesc &d, PreparedScene &s)
{
    const uint64_t n_prims64 = static_cast<uint64_t>(d.n_tris) + d.n_spheres;
    if (!d.width || !d.height || !n_prims64 || !d.samples || !d.n_samples || !d.nb_ray) return RTX_ERR_BAD_ARG;
    if ((d.n_tris && (!d.v0v1v2 || !d.rgb)) || (d.n_spheres && (!d.spheres || !d.sphere_rgb))) return RTX_ERR_BAD_ARG;
    if (n_prims64 > kLeafIndexMask || d.accel > RTX_ACCEL_BRUTE || d.reference_tree > RTX_REFTREE_NEVER) return RTX_ERR_BAD_ARG;
    // the walk addresses records by 32-bit byte offsets (64 B per primitive, 32 B per node, < 2 nodes per primitive)
    if (n_prims64 >= kMaxPrimitives) return RTX_ERR_UNSUPPORTED;
    if (static_cast<uint64_t>(d.width) * d.height >= (1ull << 31)) return RTX_ERR_BAD_ARG;
    const uint32_t n_prims = static_cast<uint32_t>(n_prims64);
    if (d.kinds) {
        uint64_t ones = 0;
        for (uint32_t i = 0; i < n_prims; ++i) ones += d.kinds[i] != 0;
        if (ones != d.n_spheres) return RTX_ERR_BAD_ARG;
    }

    s.width = d.width;
    s.height = d.height;
    std::memcpy(s.eye, d.eye, 12);
    std::memcpy(s.cam_u, d.u, 12);
    std::memcpy(s.cam_v, d.v, 12);
    std::memcpy(s.cam_w, d.w, 12);
    s.distance = d.distance;
    s.nb_ray = d.nb_ray;
    s.nb_light_sample = d.nb_light_sample;
    s.n_tris = n_prims;
    s.n_spheres = d.n_spheres;
    s.n_samples = d.n_samples;
    try {
        s.samples.assign(d.samples, d.samples + 2 * static_cast<size_t>(d.n_samples));

        std::memcpy(s.light_v, d.light_v0, 12);
        std::memcpy(s.light_v + 3, d.light_v1, 12);
        std::memcpy(s.light_v + 6, d.light_v2, 12);
        s.seeded = false;
        s.sample_seed = 0;
        s.table_generation = 0;
        light_walk_of(s.light_v, SampleSource{d.samples, 0, d.n_samples}, d.nb_ray, d.nb_light_sample, s.light_points,
                      s.light_tour, s.light_order, s.light_boxes);

        const int grc = build_gamma_thresholds(s.gamma_thr);
        if (grc != RTX_OK) return grc;

        // primitive records in the order of the caller's Vec<Primitive> (kinds), both arms
        std::vector<Prim> prims(n_prims);
        std::vector<TriRec> recs(n_prims);
        std::vector<float> boxes(6 * static_cast<size_t>(n_prims));
        s.shade.resize(n_prims);
        // the rest geometry of rtx_scene_pose_moved: the arrays as given, and each entry's position in the Vec
        if (d.n_tris) s.rest_v0v1v2.assign(d.v0v1v2, d.v0v1v2 + 9 * static_cast<size_t>(d.n_tris));
        if (d.n_spheres) s.rest_spheres.assign(d.spheres, d.spheres + 4 * static_cast<size_t>(d.n_spheres));
        s.rest_tri_vec.clear();
        s.rest_sphere_vec.clear();
        s.rest_tri_vec.reserve(d.n_tris);
        s.rest_sphere_vec.reserve(d.n_spheres);
        uint32_t next_tri = 0, next_sphere = 0;
        for (uint32_t i = 0; i < n_prims; ++i) {
            const bool sphere = d.kinds ? d.kinds[i] != 0 : i >= d.n_tris;
            (sphere ? s.rest_sphere_vec : s.rest_tri_vec).push_back(i);
            TriRec &r = recs[i];
            ShadeRec &sh = s.shade[i];
            std::memset(&r, 0, sizeof r);
            if (sphere) {
                const float *p = d.spheres + 4 * static_cast<size_t>(next_sphere);
                for (int k = 0; k < 4; ++k)
                    if (!std::isfinite(p[k])) return RTX_ERR_UNSUPPORTED;
                sphere_statement(p, r.v0, r.e1, r.bmin, r.bmax, sh.normal);  // Sphere::new, get_bounding_box (scene_prep.h)
                std::memcpy(sh.rgb, d.sphere_rgb + 3 * static_cast<size_t>(next_sphere), 12);
                sh.kind = 1;
                ++next_sphere;
            } else {
                const float *t = d.v0v1v2 + 9 * static_cast<size_t>(next_tri);
                for (int k = 0; k < 9; ++k)
                    if (!std::isfinite(t[k])) return RTX_ERR_UNSUPPORTED;
                std::memcpy(r.v0, t, 12);
                triangle_derive(t, t + 3, t + 6, r.e1, r.e2, sh.normal, r.bmin, r.bmax);
                std::memcpy(sh.rgb, d.rgb + 3 * static_cast<size_t>(next_tri), 12);
                sh.kind = 0;
                ++next_tri;
            }
            r.idx = i;
            std::memcpy(&boxes[6 * static_cast<size_t>(i)], r.bmin, 12);
            std::memcpy(&boxes[6 * static_cast<size_t>(i) + 3], r.bmax, 12);
            Prim &p = prims[i];
            for (int k = 0; k < 3; ++k) {
                p.lo[k] = r.bmin[k];
                p.hi[k] = r.bmax[k];
                p.c[k] = 0.5f * r.bmin[k] + 0.5f * r.bmax[k];
            }
            p.idx = i;
            p.kind = sphere ? 1u : 0u;
        }

        {   // PreparedScene::cull_delta
            float magnitude = 0.0f;
            for (float b : boxes) magnitude = std::fmax(magnitude, std::fabs(b));
            for (int k = 0; k < 3; ++k) magnitude = std::fmax(magnitude, std::fabs(d.eye[k]));
            s.cull_delta = magnitude * 0x1p-19f + 0x1p-100f;
            if (!std::isfinite(s.cull_delta)) return RTX_ERR_UNSUPPORTED;
            // PreparedScene::shaft_delta: the same with the light points counted in (a shaft ends on them)
            s.scene_magnitude = magnitude;
            s.shaft_delta = shaft_delta_of(magnitude, s.light_boxes.data(), s.light_boxes.size());
            if (!std::isfinite(s.shaft_delta)) return RTX_ERR_UNSUPPORTED;
        }

        // the reference's own tree (see ref_tree_build): ranks for exact ties, stream for hard directions
        std::vector<uint32_t> ref_rank;
        s.ref_nodes.clear();
        const bool want_ref = d.reference_tree == RTX_REFTREE_ALWAYS ||
                              (d.reference_tree == RTX_REFTREE_AUTO && n_prims <= kRefTreeAutoMax);
        if (want_ref) {
            ref_rank.resize(n_prims);
            const int rrc = ref_tree_build_boxes(n_prims, boxes.data(), ref_rank.data(), &s.ref_nodes);
            if (rrc != RTX_OK) return rrc;
        }
        for (uint32_t i = 0; i < n_prims; ++i)
            s.shade[i].rank = d.tie_rank ? d.tie_rank[i] : (want_ref ? ref_rank[i] : i);

        // after a tree is built: inner nodes of the library's stream name their second child in `info` (the first one
        // is the next record; the walks only look at bit 31 of an inner node's info, the cut's descent follows both).
        auto finish_tree = [&]() {
            for (size_t i = 0; i < s.nodes.size(); ++i)
                if (!(s.nodes[i].info & kLeafFlag)) {
                    const NodeRec &first = s.nodes[i + 1];
                    s.nodes[i].info = (first.info & kLeafFlag) ? static_cast<uint32_t>(i) + 2u : first.link;
                }
        };
        s.nodes.clear();
        s.primary_nodes.clear();
        s.nodes.reserve(2 * static_cast<size_t>(n_prims));
        s.leaf_max = d.leaf_max ? d.leaf_max : 4;          // (a rebuilt pose's: rebuild_tables)
        if (d.accel == RTX_ACCEL_BRUTE) {
            // one leaf per arm (a leaf holds one arm only), under a root when both are present
            auto it = std::stable_partition(prims.begin(), prims.end(), [](const Prim &p) { return p.kind == 0u; });
            const uint32_t n_tri_prims = static_cast<uint32_t>(it - prims.begin());
            auto leaf_of = [&](uint32_t begin, uint32_t end) {
                Box b;
                b.reset();
                for (uint32_t i = begin; i < end; ++i) b.grow(prims[i].lo, prims[i].hi);
                NodeRec rec;
                std::memcpy(rec.bmin, b.lo, 12);
                std::memcpy(rec.bmax, b.hi, 12);
                rec.info = kLeafFlag | (prims[begin].kind ? kSphereFlag : 0u) | begin;
                rec.link = end - begin;
                return rec;
            };
            if (n_tri_prims == 0 || n_tri_prims == n_prims) {
                s.nodes.push_back(leaf_of(0, n_prims));
            } else {
                const NodeRec a = leaf_of(0, n_tri_prims), b = leaf_of(n_tri_prims, n_prims);
                Box all;
                all.reset();
                all.grow(a.bmin, a.bmax);
                all.grow(b.bmin, b.bmax);
                NodeRec root;
                std::memcpy(root.bmin, all.lo, 12);
                std::memcpy(root.bmax, all.hi, 12);
                root.info = 0;
                root.link = 3;
                s.nodes.push_back(root);
                s.nodes.push_back(a);
                s.nodes.push_back(b);
            }
            s.n_global = 0;
            s.n_leaves = static_cast<uint32_t>(s.nodes.size() == 1 ? 1 : 2);
            s.max_leaf_tris = std::max(n_tri_prims, n_prims - n_tri_prims);
            s.depth = s.nodes.size() == 1 ? 1 : 2;
            finish_tree();
        } else {
            uint32_t leaf_max = d.leaf_max ? d.leaf_max : 4;
            double box_cost = 1.0;
            bool global_leaf = true;
#if RTX_ABLATION   // sweeps of tools/sweep.py; librtx.so takes these from RtxSceneDesc (leaf_max) or not at all
            if (const char *e = std::getenv("RTX_LEAF_MAX")) leaf_max = std::max(1, std::atoi(e));
            if (const char *e = std::getenv("RTX_SAH_BOX_COST")) { const double c = std::atof(e); if (c > 0.0) box_cost = c; }
            global_leaf = !std::getenv("RTX_NO_GLOBAL_LEAF");
#endif
            // "Global" primitives: triangles whose own box is about as large as the scene's (the ground of main()).
            // Every ray meets such a box, so testing it is wasted work, and as a child of the root it makes the root's
            // other child — the actual scene — one level deeper for everybody.  They go into the first leaf, which
            // the walk processes up front without a box test (acceptance without a test is always sound: culling is
            // a superset), under a root that is never tested either; the tree proper hangs beside it.
            s.n_global = 0;
            Box all;
            all.reset();
            for (const Prim &p : prims) all.grow(p.lo, p.hi);
            const double scene_area = all.half_area();
            if (scene_area > 0 && global_leaf) {
                auto is_global = [&](const Prim &p) {
                    Box b;
                    std::memcpy(b.lo, p.lo, 12);
                    std::memcpy(b.hi, p.hi, 12);
                    return p.kind == 0u && b.half_area() >= 0.5 * scene_area;
                };
                const size_t n = static_cast<size_t>(std::count_if(prims.begin(), prims.end(), is_global));
                if (n >= 1 && n <= kMaxGlobalPrims) {
                    std::stable_partition(prims.begin(), prims.end(), is_global);
                    s.n_global = static_cast<uint32_t>(n);
                }
            }
            // centre of the light points (the first primary ray's): orders the children of every node (TreeBuilder)
            float light_c[3] = {0.0f, 0.0f, 0.0f};
            bool light_ok = d.nb_light_sample != 0u;
            if (light_ok) {
                double acc[3] = {0, 0, 0};
                for (uint32_t i = 0; i < d.nb_light_sample; ++i)
                    for (int k = 0; k < 3; ++k) acc[k] += s.light_points[3 * static_cast<size_t>(i) + k];
                for (int k = 0; k < 3; ++k) {
                    light_c[k] = static_cast<float>(acc[k] / d.nb_light_sample);
                    light_ok = light_ok && std::isfinite(light_c[k]);
                }
            }
            {
                TreeBuilder tb(prims, s.nodes, leaf_max, box_cost, 64u, light_ok ? light_c : nullptr);
                if (s.n_global) {
                    Box g;
                    g.reset();
                    for (uint32_t i = 0; i < s.n_global; ++i) g.grow(prims[i].lo, prims[i].hi);
                    NodeRec leaf;
                    std::memcpy(leaf.bmin, g.lo, 12);
                    std::memcpy(leaf.bmax, g.hi, 12);
                    leaf.info = kLeafFlag | 0u;
                    leaf.link = s.n_global;
                    if (s.n_global < n_prims) {
                        NodeRec root;
                        std::memcpy(root.bmin, all.lo, 12);
                        std::memcpy(root.bmax, all.hi, 12);
                        root.info = 0;
                        root.link = 0;
                        s.nodes.push_back(root);
                        s.nodes.push_back(leaf);
                        tb.build(s.n_global, n_prims, 1);
                        s.nodes[0].link = static_cast<uint32_t>(s.nodes.size());
                    } else {
                        s.nodes.push_back(leaf);
                    }
                    s.n_leaves = tb.leaves + 1;
                    s.max_leaf_tris = tb.max_leaf;          // of the tree proper; the global leaf holds n_global
                    s.depth = tb.depth + 1;
                } else {
                    tb.build(0, n_prims, 0);
                    s.n_leaves = tb.leaves;
                    s.max_leaf_tris = tb.max_leaf;
                    s.depth = tb.depth;
                }
            }
            finish_tree();
            s.primary_nodes.clear();
            if (s.n_global < n_prims)
                stream_nearest_first(s.nodes, s.n_global != 0u ? 2u : 0u, d.eye, s.primary_nodes);
        }
        s.tris.resize(n_prims);
        std::vector<uint32_t> pos_of(n_prims);
        for (uint32_t i = 0; i < n_prims; ++i) {
            s.tris[i] = recs[prims[i].idx];
            pos_of[prims[i].idx] = i;
        }
        // Plane data of the global triangles (rtx_traverse.hpp: plane_rules_out): scene_prep.h's global_plane_statement,
        // the text the device compiles for a pose's triangles
        s.global_planes.assign(s.n_global, TriRec{});
        for (uint32_t i = 0; i < s.n_global; ++i) global_plane_statement(s.tris[i], &s.global_planes[i]);
        for (NodeRec &nd : s.ref_nodes)   // leaves of the reference stream point at the same record array
            if (nd.info & kLeafFlag) {
                const uint32_t prim = nd.info & kLeafIndexMask;
                nd.info = kLeafFlag | (s.shade[prim].kind ? kSphereFlag : 0u) | pos_of[prim];
            }
        // range of the sample table (the jitter of the primary rays), then the long primary walks (scene_prep.h)
        for (int c = 0; c < 2; ++c) {
            float lo = d.samples[c], hi = d.samples[c];
            bool finite = true;
            for (size_t i = 0; i < d.n_samples; ++i) {
                const float v = d.samples[2 * i + c];
                finite = finite && std::isfinite(v);
                lo = v < lo ? v : lo;
                hi = v > hi ? v : hi;
            }
            s.sample_lo[c] = finite ? lo : std::nanf("");
            s.sample_hi[c] = finite ? hi : std::nanf("");
        }
        predict_long_tiles(s, kProbeLongWeight);
    } catch (const std::bad_alloc &) {
        return RTX_ERR_OOM;
    }
    return RTX_OK;
}

// ---- the long primary walks (scene_prep.h) ------------------------------------------------------------------------------

namespace {

// The primary stream's boxes as uploaded (nodes_in_device_order: each plane moved by cull_delta in f32), in double, and
// the walk of the stream against one tile's frustum.
struct ProbePredictor {
    const PreparedScene &s;
    const std::vector<NodeRec> &stream;
    std::vector<double> box;           // n x {lo xyz, hi xyz}, relative to the eye
    uint32_t root = 0;
    bool usable = false;
    explicit ProbePredictor(const PreparedScene &scene)
        : s(scene), stream(scene.primary_nodes.empty() ? scene.nodes : scene.primary_nodes)
    {
        root = (s.n_global != 0u && stream.size() > 2u) ? 2u : (s.n_global != 0u ? static_cast<uint32_t>(stream.size()) : 0u);
        usable = stream.size() <= kProbeSplitMaxNodes && s.width && s.height;
        for (int c = 0; c < 2; ++c) usable = usable && std::isfinite(s.sample_lo[c]) && std::isfinite(s.sample_hi[c]);
        if (!usable) return;
        box.resize(6 * stream.size());
        for (size_t i = 0; i < stream.size(); ++i)
            for (int k = 0; k < 3; ++k) {
                box[6 * i + k] = static_cast<double>(stream[i].bmin[k] - s.cull_delta) - static_cast<double>(s.eye[k]);
                box[6 * i + 3 + k] = static_cast<double>(stream[i].bmax[k] + s.cull_delta) - static_cast<double>(s.eye[k]);
            }
    }
    // the four planes through the eye around the tile's rays, normals pointing inwards; false: no proper frustum
    bool planes_of(uint32_t tile_x, uint32_t tile_y, double n[4][3]) const
    {
        // create_rays: a = px - W / 2 + s0, b = py - H / 2 + s1 over the tile's pixels and the table's range, one more
        // pixel each side (the kernel rounds a and b to f32: 2^-12 of a pixel at most)
        const double lo0 = std::fmin(static_cast<double>(s.sample_lo[0]), 0.0), hi0 = std::fmax(static_cast<double>(s.sample_hi[0]), 1.0);
        const double lo1 = std::fmin(static_cast<double>(s.sample_lo[1]), 0.0), hi1 = std::fmax(static_cast<double>(s.sample_hi[1]), 1.0);
        const double a0 = 8.0 * tile_x - 0.5 * s.width + lo0 - 1.0, a1 = 8.0 * tile_x + 7.0 - 0.5 * s.width + hi0 + 1.0;
        const double b0 = 8.0 * tile_y - 0.5 * s.height + lo1 - 1.0, b1 = 8.0 * tile_y + 7.0 - 0.5 * s.height + hi1 + 1.0;
        auto dir = [&](double a, double b, double out[3]) {
            for (int k = 0; k < 3; ++k)
                out[k] = a * s.cam_u[k] + b * s.cam_v[k] - static_cast<double>(s.distance) * s.cam_w[k];
        };
        double c[4][3], mid[3];
        dir(a0, b0, c[0]); dir(a1, b0, c[1]); dir(a1, b1, c[2]); dir(a0, b1, c[3]);
        dir(0.5 * (a0 + a1), 0.5 * (b0 + b1), mid);
        for (int e = 0; e < 4; ++e) {
            const double *p = c[e], *q = c[(e + 1) % 4];
            n[e][0] = p[1] * q[2] - p[2] * q[1];
            n[e][1] = p[2] * q[0] - p[0] * q[2];
            n[e][2] = p[0] * q[1] - p[1] * q[0];
            double inside = n[e][0] * mid[0] + n[e][1] * mid[1] + n[e][2] * mid[2];
            if (inside < 0.0) {
                for (int k = 0; k < 3; ++k) n[e][k] = -n[e][k];
                inside = -inside;
            }
            if (!(inside > 0.0) || !std::isfinite(inside)) return false;
        }
        return true;
    }
    // a box lies outside when all of it is behind one plane: its corner farthest along the normal decides
    bool meets(const double n[4][3], size_t i) const
    {
        const double *b = &box[6 * i];
        for (int e = 0; e < 4; ++e) {
            double far = 0.0;
            for (int k = 0; k < 3; ++k) far += n[e][k] * (n[e][k] > 0.0 ? b[3 + k] : b[k]);
            if (far < 0.0) return false;        // (a NaN keeps the box)
        }
        return true;
    }
    uint32_t weigh(uint32_t tile_x, uint32_t tile_y, uint8_t *met, bool *valid) const
    {
        double n[4][3];
        *valid = usable && planes_of(tile_x, tile_y, n);
        if (!*valid) return 0u;
        if (met)
            for (uint32_t i = 0; i < root && i < stream.size(); ++i) met[i] = 1;
        uint64_t w = 0;
        for (size_t i = root; i < stream.size();) {
            const NodeRec &nd = stream[i];
            const bool leaf = (nd.info & kLeafFlag) != 0u;
            const bool pass = meets(n, i);
            if (pass) {
                w += leaf ? 1u + 3ull * nd.link : 1u;
                if (met) met[i] = 1;
            }
            i = (leaf || pass) ? i + 1 : (nd.link > i ? nd.link : stream.size());
        }
        return w > 0xFFFFFFFFull ? 0xFFFFFFFFu : static_cast<uint32_t>(w);
    }
};

}  // namespace

uint32_t probe_tile_weight(const PreparedScene &s, uint32_t tile_x, uint32_t tile_y, uint8_t *met, bool *valid)
{
    const ProbePredictor p(s);
    return p.weigh(tile_x, tile_y, met, valid);
}

void predict_long_tiles(PreparedScene &s, uint32_t threshold)
{
    s.long_tiles.clear();
    s.long_weights.clear();
    s.long_bits.clear();
    const ProbePredictor p(s);
    if (!p.usable) return;
    const uint32_t tiles_x = (s.width + 7u) / 8u, tiles_y = (s.height + 7u) / 8u;
    const uint64_t n_tiles64 = static_cast<uint64_t>(tiles_x) * tiles_y;
    if (n_tiles64 > 0x7FFFFFFFull) return;
    const uint32_t n_tiles = static_cast<uint32_t>(n_tiles64), cap = probe_long_cap(n_tiles);
    if (cap == 0u) return;
    std::vector<std::pair<uint32_t, uint32_t>> found;     // (weight, tile)
    for (uint32_t ty = 0; ty < tiles_y; ++ty)
        for (uint32_t tx = 0; tx < tiles_x; ++tx) {
            bool valid = false;
            const uint32_t w = p.weigh(tx, ty, nullptr, &valid);
            if (!valid) return;                            // one improper frustum: no prediction for the scene
            if (w >= threshold) found.emplace_back(w, ty * tiles_x + tx);
        }
    // costliest first, equal weights by tile number: one order whatever the sort does with ties
    std::sort(found.begin(), found.end(), [](const std::pair<uint32_t, uint32_t> &a, const std::pair<uint32_t, uint32_t> &b) {
        return a.first != b.first ? a.first > b.first : a.second < b.second;
    });
    if (found.size() > cap) found.resize(cap);
    if (found.size() < kProbeLongMinTiles) return;
    s.long_bits.assign((n_tiles + 31u) / 32u, 0u);
    for (const auto &f : found) {
        s.long_tiles.push_back(f.second);
        s.long_weights.push_back(f.first);
        s.long_bits[f.second >> 5] |= 1u << (f.second & 31u);
    }
}

// ---- posing (scene_prep.h) ----------------------------------------------------------------------------------------------

void pose_tables(const PreparedScene &s, PoseTables &out)
{
    const size_t n_nodes = s.nodes.size(), n_prims = s.shade.size();
    out.ranges.assign(2u * n_nodes, 0u);
    for (size_t i = n_nodes; i-- > 0;) {        // pre-order: both children of an inner node lie behind it
        const NodeRec &n = s.nodes[i];
        uint32_t first, end;
        if (n.info & kLeafFlag) {
            first = n.info & kLeafIndexMask;
            end = first + n.link;
        } else {
            const size_t a = i + 1u, b = n.info;
            first = std::min(out.ranges[2u * a], out.ranges[2u * b]);
            end = std::max(out.ranges[2u * a] + out.ranges[2u * a + 1u], out.ranges[2u * b] + out.ranges[2u * b + 1u]);
        }
        out.ranges[2u * i] = first;
        out.ranges[2u * i + 1u] = end - first;
    }
    out.tri_of.assign(n_prims, kPoseNoTriangle);
    out.sphere_of.assign(n_prims, kPoseNoTriangle);
    uint32_t next = 0, next_sphere = 0;
    for (size_t i = 0; i < n_prims; ++i) {
        if (s.shade[i].kind == 0u) out.tri_of[i] = next++;
        else out.sphere_of[i] = next_sphere++;
    }
    out.order.clear();
    out.order.reserve(n_nodes);
    for (uint32_t i = 0; i < n_nodes; ++i)
        if (out.ranges[2u * i + 1u] > kPoseLaneMax) out.order.push_back(i);
    out.n_long = static_cast<uint32_t>(out.order.size());
    for (uint32_t i = 0; i < n_nodes; ++i)
        if (out.ranges[2u * i + 1u] <= kPoseLaneMax) out.order.push_back(i);
}

bool pose_in_range(const PreparedScene &s, const float *pose)
{
    const size_t n = 9u * static_cast<size_t>(s.n_tris - s.n_spheres);
    for (size_t k = 0; k < n; ++k)
        if (!(std::fabs(pose[k]) <= s.scene_magnitude)) return false;      // (false for a NaN)
    return true;
}

namespace {
bool sphere_in_range(const PreparedScene &s, const float *p)
{
    float v0[3], e1[3], lo[3], hi[3], origin[3];
    for (int k = 0; k < 4; ++k)
        if (!std::isfinite(p[k])) return false;
    sphere_statement(p, v0, e1, lo, hi, origin);
    for (int k = 0; k < 3; ++k)
        if (!(std::fabs(lo[k]) <= s.scene_magnitude) || !(std::fabs(hi[k]) <= s.scene_magnitude)) return false;
    return true;
}
}  // namespace

bool spheres_in_range(const PreparedScene &s, const float *spheres)
{
    for (size_t i = 0; i < s.n_spheres; ++i)
        if (!sphere_in_range(s, spheres + 4u * i)) return false;
    return true;
}

void moved_prims(const PreparedScene &s, const PoseMoves &m, float *out_v0v1v2, float *out_spheres)
{
    if (out_v0v1v2)
        for (size_t t = 0; t < s.rest_tri_vec.size(); ++t) {
            const uint32_t g = m.group ? m.group[s.rest_tri_vec[t]] : 0u;
            for (size_t k = 0; k < 3u; ++k)
                move_statement(m.moves, m.radius_scale, m.n_moves, g, false, &s.rest_v0v1v2[9u * t + 3u * k], out_v0v1v2 + 9u * t + 3u * k);
        }
    if (out_spheres)
        for (size_t i = 0; i < s.rest_sphere_vec.size(); ++i) {
            const uint32_t g = m.group ? m.group[s.rest_sphere_vec[i]] : 0u;
            move_statement(m.moves, m.radius_scale, m.n_moves, g, true, &s.rest_spheres[4u * i], out_spheres + 4u * i);
        }
}

bool moved_in_range(const PreparedScene &s, const PoseMoves &m)
{
    for (size_t t = 0; t < s.rest_tri_vec.size(); ++t) {
        const uint32_t g = m.group ? m.group[s.rest_tri_vec[t]] : 0u;
        for (size_t k = 0; k < 3u; ++k) {
            float out[3];
            move_statement(m.moves, m.radius_scale, m.n_moves, g, false, &s.rest_v0v1v2[9u * t + 3u * k], out);
            for (int c = 0; c < 3; ++c)
                if (!(std::fabs(out[c]) <= s.scene_magnitude)) return false;      // (false for a NaN)
        }
    }
    for (size_t i = 0; i < s.rest_sphere_vec.size(); ++i) {
        float out[4];
        move_statement(m.moves, m.radius_scale, m.n_moves, m.group ? m.group[s.rest_sphere_vec[i]] : 0u, true, &s.rest_spheres[4u * i], out);
        if (!sphere_in_range(s, out)) return false;
    }
    return true;
}

bool move_groups_ok(const PreparedScene &s, const PoseMoves &m)
{
    if (!m.group) return true;
    for (size_t i = 0; i < s.n_tris; ++i)
        if (m.group[i] >= m.n_moves && m.group[i] != kMoveNone) return false;
    return true;
}

int skin_bind(const PreparedScene &s, const uint32_t *bones, const float *weights, const uint32_t *sphere_bone, Skin &out)
{
    const size_t n_corner_words = 12u * s.rest_tri_vec.size(), n_spheres = s.rest_sphere_vec.size();
    if (n_corner_words && (!bones || !weights)) return RTX_ERR_BAD_ARG;
    for (size_t k = 0; k < n_corner_words; ++k)
        if (!std::isfinite(weights[k])) return RTX_ERR_UNSUPPORTED;
    Skin made;
    try {
        if (n_corner_words) {
            made.bones.assign(bones, bones + n_corner_words);
            made.weights.assign(weights, weights + n_corner_words);
        }
        if (sphere_bone) made.sphere_bone.assign(sphere_bone, sphere_bone + n_spheres);
        else made.sphere_bone.assign(n_spheres, kMoveNone);
    } catch (...) {
        return RTX_ERR_OOM;
    }
    for (uint32_t b : made.bones)
        if (b != kMoveNone && b > made.max_bone) made.max_bone = b;
    for (uint32_t b : made.sphere_bone)
        if (b != kMoveNone && b > made.max_bone) made.max_bone = b;
    made.bound = true;
    made.generation = out.generation + 1u;
    out = std::move(made);
    return RTX_OK;
}

void skinned_prims(const PreparedScene &s, const Skin &skin, const PoseMoves &m, float *out_v0v1v2, float *out_spheres)
{
    if (out_v0v1v2)
        for (size_t c = 0; c < 3u * s.rest_tri_vec.size(); ++c)
            skin_statement(m.moves, m.n_moves, &skin.bones[4u * c], &skin.weights[4u * c], &s.rest_v0v1v2[3u * c], out_v0v1v2 + 3u * c);
    if (out_spheres)
        for (size_t i = 0; i < s.rest_sphere_vec.size(); ++i)
            move_statement(m.moves, m.radius_scale, m.n_moves, skin.sphere_bone[i], true, &s.rest_spheres[4u * i], out_spheres + 4u * i);
}

bool skinned_in_range(const PreparedScene &s, const Skin &skin, const PoseMoves &m)
{
    for (size_t c = 0; c < 3u * s.rest_tri_vec.size(); ++c) {
        float out[3];
        skin_statement(m.moves, m.n_moves, &skin.bones[4u * c], &skin.weights[4u * c], &s.rest_v0v1v2[3u * c], out);
        for (int k = 0; k < 3; ++k)
            if (!(std::fabs(out[k]) <= s.scene_magnitude)) return false;      // (false for a NaN)
    }
    for (size_t i = 0; i < s.rest_sphere_vec.size(); ++i) {
        float out[4];
        move_statement(m.moves, m.radius_scale, m.n_moves, skin.sphere_bone[i], true, &s.rest_spheres[4u * i], out);
        if (!sphere_in_range(s, out)) return false;
    }
    return true;
}

void overlay_records(const PreparedScene &s, const PoseTables &t, const PrimsOverlay &ov, TriRec *tris, ShadeRec *shade)
{
    const size_t n_prims = s.tris.size();
    for (size_t j = 0; j < n_prims; ++j) {
        TriRec r = s.tris[j];
        ShadeRec sh = s.shade[r.idx];
        if (sh.kind != 0u) {
            const size_t n = t.sphere_of[r.idx];
            if (ov.spheres) sphere_statement(ov.spheres + 4u * n, r.v0, r.e1, r.bmin, r.bmax, sh.normal);
            if (ov.sphere_rgb) std::memcpy(sh.rgb, ov.sphere_rgb + 3u * n, 12);
        } else if (ov.rgb) {
            std::memcpy(sh.rgb, ov.rgb + 3u * static_cast<size_t>(t.tri_of[r.idx]), 12);
        }
        if (tris) tris[j] = r;
        if (shade) shade[r.idx] = sh;
    }
}

void posed_records(const PreparedScene &s, const PoseTables &t, const float *pose, const uint32_t *rank, TriRec *tris,
                   ShadeRec *shade, NodeRec *nodes, const PrimsOverlay *ov)
{
    const size_t n_prims = s.tris.size();
    std::vector<TriRec> own;
    if (!tris) {
        own.resize(n_prims);
        tris = own.data();
    }
    // what the kernels are handed as the uploaded arrays: the scene's, or the overlay's over them
    const TriRec *in_tris = s.tris.data();
    const ShadeRec *in_shade = s.shade.data();
    std::vector<TriRec> ov_tris;
    std::vector<ShadeRec> ov_shade;
    if (ov && ov->any()) {
        ov_tris.resize(n_prims);
        ov_shade.resize(n_prims);
        overlay_records(s, t, *ov, ov_tris.data(), ov_shade.data());
        in_tris = ov_tris.data();
        in_shade = ov_shade.data();
    }
    for (size_t j = 0; j < n_prims; ++j) {
        TriRec r = in_tris[j];
        ShadeRec sh = in_shade[r.idx];
        if (sh.kind == 0u) {
            const float *v = pose + 9u * static_cast<size_t>(t.tri_of[r.idx]);
            std::memcpy(r.v0, v, 12);
            triangle_statement(v, v + 3, v + 6, r.e1, r.e2, sh.normal, r.bmin, r.bmax);
        }
        sh.rank = rank ? rank[r.idx] : r.idx;
        tris[j] = r;
        if (shade) shade[r.idx] = sh;
    }
    if (!nodes) return;
    const float inf = std::numeric_limits<float>::infinity();
    for (size_t i = 0; i < s.nodes.size(); ++i) {
        NodeRec n = s.nodes[i];
        const uint32_t first = t.ranges[2u * i], count = t.ranges[2u * i + 1u];
        for (int k = 0; k < 3; ++k) {
            float lo = inf, hi = -inf;
            for (uint32_t j = first; j < first + count; ++j) {
                lo = fminf(lo, tris[j].bmin[k]);
                hi = fmaxf(hi, tris[j].bmax[k]);
            }
            n.bmin[k] = lo - s.cull_delta;
            n.bmax[k] = hi + s.cull_delta;
        }
        nodes[i] = n;
    }
}

int posed_ref_tree(const PreparedScene &s, const PoseTables &t, const float *pose, std::vector<uint32_t> &rank,
                   std::vector<NodeRec> &stream, const PrimsOverlay *ov)
{
    const size_t n_prims = s.tris.size();
    std::vector<TriRec> tris(n_prims);
    posed_records(s, t, pose, nullptr, tris.data(), nullptr, nullptr, ov);
    std::vector<float> boxes(6u * n_prims);
    std::vector<uint32_t> pos_of(n_prims);
    for (size_t j = 0; j < n_prims; ++j) {
        const uint32_t idx = tris[j].idx;
        std::memcpy(&boxes[6u * idx], tris[j].bmin, 12);
        std::memcpy(&boxes[6u * idx + 3u], tris[j].bmax, 12);
        pos_of[idx] = static_cast<uint32_t>(j);
    }
    rank.assign(n_prims, 0u);
    const int rc = ref_tree_build_boxes(static_cast<uint32_t>(n_prims), boxes.data(), rank.data(), &stream);
    if (rc != RTX_OK) return rc;
    for (NodeRec &nd : stream)
        if (nd.info & kLeafFlag) {
            const uint32_t prim = nd.info & kLeafIndexMask;
            nd.info = kLeafFlag | (s.shade[prim].kind ? kSphereFlag : 0u) | pos_of[prim];
        }
    return RTX_OK;
}


// ---- a pose whose tree is rebuilt (scene_prep.h) ---------------------------------------------------------------------------

namespace {

// pre-order, balanced: a run of more than leaf_max records splits at begin + count / 2
void rebuild_subtree(std::vector<NodeRec> &nodes, std::vector<uint32_t> &ranges, uint32_t begin, uint32_t count, bool sphere,
                     uint32_t leaf_max)
{
    const size_t self = nodes.size();
    nodes.push_back(NodeRec{});
    ranges.push_back(begin);
    ranges.push_back(count);
    if (count <= leaf_max) {
        nodes[self].info = kLeafFlag | (sphere ? kSphereFlag : 0u) | begin;
        nodes[self].link = count;
        return;
    }
    const uint32_t half = count / 2u;
    rebuild_subtree(nodes, ranges, begin, half, sphere, leaf_max);
    nodes[self].info = static_cast<uint32_t>(nodes.size());
    rebuild_subtree(nodes, ranges, begin + half, count - half, sphere, leaf_max);
    nodes[self].link = static_cast<uint32_t>(nodes.size());
}

}  // namespace

void rebuild_tables(const PreparedScene &s, RebuildTables &out)
{
    const uint32_t n_prims = static_cast<uint32_t>(s.tris.size()), n_global = s.n_global;
    const uint32_t leaf_max = s.leaf_max ? s.leaf_max : 1u;
    uint32_t n_spheres = 0;
    for (uint32_t j = n_global; j < n_prims; ++j) n_spheres += s.shade[s.tris[j].idx].kind != 0u;
    const uint32_t n_tris = n_prims - n_global - n_spheres;
    out.n_tree_tris = n_tris;
    out.n_tree_spheres = n_spheres;
    out.nodes.clear();
    out.ranges.clear();
    auto proper = [&]() {
        if (n_tris != 0u && n_spheres != 0u) {
            const size_t self = out.nodes.size();
            out.nodes.push_back(NodeRec{});
            out.ranges.push_back(n_global);
            out.ranges.push_back(n_tris + n_spheres);
            rebuild_subtree(out.nodes, out.ranges, n_global, n_tris, false, leaf_max);
            out.nodes[self].info = static_cast<uint32_t>(out.nodes.size());
            rebuild_subtree(out.nodes, out.ranges, n_global + n_tris, n_spheres, true, leaf_max);
            out.nodes[self].link = static_cast<uint32_t>(out.nodes.size());
        } else if (n_tris != 0u) {
            rebuild_subtree(out.nodes, out.ranges, n_global, n_tris, false, leaf_max);
        } else if (n_spheres != 0u) {
            rebuild_subtree(out.nodes, out.ranges, n_global, n_spheres, true, leaf_max);
        }
    };
    if (n_global != 0u) {               // as prepare_scene lays them out: the root, the global leaf, the tree proper
        NodeRec leaf{};
        leaf.info = kLeafFlag | 0u;
        leaf.link = n_global;
        if (n_global < n_prims) {
            NodeRec root{};
            root.info = 2u;
            out.nodes.push_back(root);
            out.ranges.push_back(0u);
            out.ranges.push_back(n_prims);
            out.nodes.push_back(leaf);
            out.ranges.push_back(0u);
            out.ranges.push_back(n_global);
            proper();
            out.nodes[0].link = static_cast<uint32_t>(out.nodes.size());
        } else {
            out.nodes.push_back(leaf);
            out.ranges.push_back(0u);
            out.ranges.push_back(n_global);
        }
    } else {
        proper();
    }
    const uint32_t n_nodes = static_cast<uint32_t>(out.nodes.size());
    out.order.clear();
    out.order.reserve(n_nodes);
    for (uint32_t i = 0; i < n_nodes; ++i)
        if (out.ranges[2u * i + 1u] > kPoseLaneMax) out.order.push_back(i);
    out.n_long = static_cast<uint32_t>(out.order.size());
    for (uint32_t i = 0; i < n_nodes; ++i)
        if (out.ranges[2u * i + 1u] <= kPoseLaneMax) out.order.push_back(i);
}

void rebuilt_records(const PreparedScene &s, const PoseTables &t, const RebuildTables &b, const float *pose,
                     const uint32_t *rank, uint64_t *keys, uint32_t *perm, TriRec *tris, ShadeRec *shade, NodeRec *nodes,
                     const PrimsOverlay *ov)
{
    const size_t n_prims = s.tris.size(), n_global = s.n_global, n_tree = n_prims - n_global;
    std::vector<TriRec> posed(n_prims);
    posed_records(s, t, pose, rank, posed.data(), shade, nullptr, ov);
    const float scale = rebuild_key_scale(s.scene_magnitude);
    std::vector<uint64_t> key_of(n_tree);
    for (size_t p = 0; p < n_tree; ++p) {
        const TriRec &r = posed[n_global + p];
        key_of[p] = rebuild_key_statement(r.bmin, r.bmax, s.shade[r.idx].kind != 0u, s.scene_magnitude, scale);
    }
    std::vector<uint32_t> at(n_tree);
    for (size_t p = 0; p < n_tree; ++p) at[p] = static_cast<uint32_t>(p);
    std::stable_sort(at.begin(), at.end(), [&](uint32_t x, uint32_t y) { return key_of[x] < key_of[y]; });
    std::vector<TriRec> own;
    if (!tris && nodes) {
        own.resize(n_prims);
        tris = own.data();
    }
    for (size_t p = 0; p < n_tree; ++p) {
        if (keys) keys[p] = key_of[at[p]];
        if (perm) perm[p] = static_cast<uint32_t>(n_global) + at[p];
    }
    if (tris) {
        for (size_t j = 0; j < n_global; ++j) tris[j] = posed[j];
        for (size_t p = 0; p < n_tree; ++p) tris[n_global + p] = posed[n_global + at[p]];
    }
    if (!nodes) return;
    const float inf = std::numeric_limits<float>::infinity();
    for (size_t i = 0; i < b.nodes.size(); ++i) {
        NodeRec n = b.nodes[i];
        const uint32_t first = b.ranges[2u * i], count = b.ranges[2u * i + 1u];
        for (int k = 0; k < 3; ++k) {
            float lo = inf, hi = -inf;
            for (uint32_t j = first; j < first + count; ++j) {
                lo = fminf(lo, tris[j].bmin[k]);
                hi = fmaxf(hi, tris[j].bmax[k]);
            }
            n.bmin[k] = lo - s.cull_delta;
            n.bmax[k] = hi + s.cull_delta;
        }
        nodes[i] = n;
    }
}

int rebuilt_ref_tree(const PreparedScene &s, const PoseTables &t, const float *pose, const uint32_t *perm,
                     std::vector<uint32_t> &rank, std::vector<NodeRec> &stream, const PrimsOverlay *ov)
{
    const int rc = posed_ref_tree(s, t, pose, rank, stream, ov);      // its leaves name positions of the uploaded array
    if (rc != RTX_OK) return rc;
    const size_t n_prims = s.tris.size(), n_global = s.n_global;
    std::vector<uint32_t> sorted_of(n_prims);
    for (size_t j = 0; j < n_global; ++j) sorted_of[j] = static_cast<uint32_t>(j);
    for (size_t p = 0; p + n_global < n_prims; ++p) sorted_of[perm[p]] = static_cast<uint32_t>(n_global + p);
    for (NodeRec &nd : stream)
        if (nd.info & kLeafFlag) nd.info = (nd.info & ~kLeafIndexMask) | sorted_of[nd.info & kLeafIndexMask];
    return RTX_OK;
}

}  // namespace rtx
