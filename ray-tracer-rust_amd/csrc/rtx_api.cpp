// rtx_api.cpp — the C ABI of librtx.so (include/rtx.h): scene handles, uploads, launches, gathers.
//
// Stands where the thread fan-out of the reference's render() stands (src/main.rs:275-303):
// the caller has a Scene and a sample table, and gets back RGB8 rows.  No CPU rendering path
// exists in this library; without a HIP device every render entry point fails.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <type_traits>
#include <vector>

#include "../../include/rtx.h"
#include "rtx_accum.h"
#include "rtx_adapt.h"
#include "rtx_aim.h"
#include "rtx_device.h"
#include "rtx_light.h"
#include "rtx_move.h"
#include "rtx_skin.h"
#include "rtx_samples.h"
#include "rtx_planes.h"
#include "rtx_pose.h"
#include "rtx_prims.h"
#include "rtx_rebuild.h"
#include "rtx_query.h"
#include "rtx_shade.h"
#include "rtx_tour.h"
#include "rtx_view.h"
#include "scene_prep.h"

namespace {

thread_local int g_last_hip_error = 0;

// the one mapping from a HIP result to the ABI's code; a failure is kept for rtx_last_hip_error
int hip_rc(hipError_t e)
{
    if (e == hipSuccess) return RTX_OK;
    g_last_hip_error = static_cast<int>(e);
    return e == hipErrorOutOfMemory ? RTX_ERR_OOM : RTX_ERR_HIP;
}

// leave the function with the code of a step that failed: RTX_TRY for a step that gives the ABI's code, RTX_HIP for a HIP call
#define RTX_TRY(step)                          \
    do {                                       \
        const int rc_ = (step);                \
        if (rc_ != RTX_OK) return rc_;         \
    } while (0)
#define RTX_HIP(call) RTX_TRY(hip_rc(call))

// makes a device current; restores the caller's current device on scope exit
class DeviceGuard {
public:
    DeviceGuard() = default;
    explicit DeviceGuard(int dev) { (void)set(dev); }
    ~DeviceGuard() { if (ok_) (void)hipSetDevice(prev_); }
    hipError_t set(int dev) { ok_ = hipGetDevice(&prev_) == hipSuccess; return err_ = hipSetDevice(dev); }
    hipError_t status() const { return err_; }
private:
    int prev_ = 0;
    bool ok_ = false;
    hipError_t err_ = hipSuccess;
};

// ---- owners ------------------------------------------------------------------------------------------------------------
// Each holds one HIP handle and gives it back when it is destroyed, which needs the handle's device current.  They are
// meant as members of DeviceState: its destructor is private, so that nothing but ReleaseOnDevice, which makes the
// state's device current first, can run theirs.
template <class T, hipError_t (*Free)(T)>
class Owned {
public:
    Owned() = default;
    Owned(const Owned &) = delete;
    Owned &operator=(const Owned &) = delete;
    ~Owned() { (void)reset(); }
    hipError_t reset()
    {
        const hipError_t e = h_ ? Free(h_) : hipSuccess;
        h_ = nullptr;
        return e;
    }
    T *put() { return &h_; }             // for the HIP call that creates the handle, while the owner is empty
    operator T() const { return h_; }
private:
    T h_ = nullptr;
};
using Stream = Owned<hipStream_t, hipStreamDestroy>;
using Event = Owned<hipEvent_t, hipEventDestroy>;

// "The library's buffer is busy up to this point of the caller's stream": a device-resident call that used a library-owned
// buffer records the buffer's event behind its kernels (the event is made on first use), and a call that uses the buffer
// on the library's stream waits for it first.  A buffer no device-resident call has used has no event: nothing to wait for.
int mark_busy(Event &e, hipStream_t callers)
{
    if (!e) RTX_HIP(hipEventCreateWithFlags(e.put(), hipEventDisableTiming));
    RTX_HIP(hipEventRecord(e, callers));
    return RTX_OK;
}

int wait_for(const Event &e, hipStream_t stream)
{
    if (e) RTX_HIP(hipStreamWaitEvent(stream, e, 0));
    return RTX_OK;
}

hipError_t alloc_device(void **p, size_t bytes) { return hipMalloc(p, bytes); }
hipError_t alloc_pinned(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }

// Grow-only memory.  reserve(): nothing to do when it is large enough; otherwise free, then allocate — the contents are
// not preserved, and after a failure the buffer is empty.
template <hipError_t (*Alloc)(void **, size_t), hipError_t (*Free)(void *)>
class GrowOnly {
public:
    int reserve(size_t bytes)
    {
        if (cap_ >= bytes) return RTX_OK;
        cap_ = 0;
        RTX_HIP(mem_.reset());
        RTX_HIP(Alloc(mem_.put(), bytes));
        cap_ = bytes;
        return RTX_OK;
    }
    size_t capacity() const { return cap_; }
    template <class T>
    T *as() const { return static_cast<T *>(static_cast<void *>(mem_)); }
private:
    Owned<void *, Free> mem_;
    size_t cap_ = 0;
};
using DeviceBuffer = GrowOnly<alloc_device, hipFree>;
using PinnedBuffer = GrowOnly<alloc_pinned, hipHostFree>;

struct Sized { DeviceBuffer &buffer; size_t bytes; };
int reserve_all(std::initializer_list<Sized> list)
{
    for (const Sized &s : list) {
        const int rc = s.buffer.reserve(s.bytes);
        if (rc != RTX_OK) return rc;
    }
    return RTX_OK;
}

// A primary rays' stream aimed on the device (rtx_aim.hip): (n_nodes + 1) records, the last one the zeroed sentinel, the aim
// kernels' scratch, and what the stream was aimed at and on — the eye's 12 bytes and the stream.  A call with the same two
// walks it as it stands.  Nothing states which nodes it was aimed over: it belongs to one DeviceGeometry and is aimed over
// that geometry's nodes only.  The uploaded scene's nodes are written once, before anything is aimed.  The pose's nodes have
// one writer, pose_launch, which takes `valid` away before it launches: a valid stream is over the nodes as they stand.
struct AimedStream {
    DeviceBuffer nodes, links;
    float eye[3] = {0.0f, 0.0f, 0.0f};
    hipStream_t on = nullptr;
    bool valid = false;
};

// The geometry a walk reads: the node stream, the reference tree's stream and its record count, the primitive and the
// shading records, the plane records of the global triangles (none: never reserved), and the primary rays' stream aimed
// over these nodes (rtx_render_view_rows).  A DeviceState holds two: the uploaded scene's (upload_all) and its pose's
// (reserve_pose, pose_launch); geometry_of picks the one a call walks, and device_scene reads all six fields from it.
struct DeviceGeometry {
    DeviceBuffer nodes, ref_nodes, tris, shade, planes;
    uint32_t n_nodes = 0;                // records of `nodes` (a sentinel follows): the scene's, or a rebuilt pose's own count
    uint32_t n_ref_nodes = 0;
    AimedStream aimed;
};

// What a scene keeps on one device.  The argument blocks the launchers read (rtx::DeviceScene, rtx::StreamWorkspace,
// rtxq::SortBuffers) are built from these owners where a launch needs them.
class DeviceState {
public:
    explicit DeviceState(int dev) : device(dev) {}
    const int device;
    bool uploaded = false;
    size_t last_tiles = 0;               // tiles of the most recent launch (rtx_debug_tile_descs)
    unsigned long long launches = 0;
    // (destroyed from the last member to the first: the stream after the events and the memory)
    Stream stream;
    Event ev0, ev1;
    Event ring[RTX_TIMING_RING][3];      // launch start / end of the scheduling pass / launch end (rtx_launch_timings)
    Event q_sorted;                      // guards q_sort (kUsesSort)
    // the uploaded scene's geometry; its aimed stream is that of the most recent unposed rtx_render_view_rows' eye.
    // primary_nodes: the scene's own eye's stream, which only the calls that render the scene's own view walk
    DeviceGeometry geo;
    DeviceBuffer primary_nodes, samples, lights, light_tour, thr, light_boxes;
    // rtx_scene_resample / rtx_scene_reseed: the generation of the scene's sample table that `samples`, `lights`, `light_tour`
    // and `light_boxes` hold (table_upload); another one than the scene's: the first call on this device catches up
    // (ensure_uploaded) before it enqueues anything
    uint64_t table_generation = 0;
    // the scene's long list as probe_kernel reads it (rtx::ProbeSplit: the tiles, then the bits), uploaded with the scene
    // when it predicts any; long_all: every tile of the frame listed (rtx_debug_probe_split, mode 2), made at first use
    DeviceBuffer long_words, long_all;
    uint32_t n_long_all = 0;
    DeviceBuffer d_out, d_counters;
    DeviceBuffer d_redo;                 // queue of tiles for reference_tiles_kernel
    // The two-pass pipeline zeroes its counting words (d_redo's headers, ws.buckets) for the NEXT launch inside each
    // launch (rtx_pass_order.hpp: order_tiles_kernel): render_launch zeroes them (zero_launch_words) when they are not known to
    // be in that state — new or grown, used by another pipeline, a launch that failed — and counts what they have
    // served since, whose parities select the words a launch works on.
    bool launch_words_ready = false;
    uint32_t words_launches = 0, words_passes = 0;
    PinnedBuffer h_stage;
    struct { DeviceBuffer hits, pix_slot, tiles, chunks, results, acc, ctr, buckets, cut; } ws;   // streamed pipeline:
                                                                                    // intermediate products in HBM
    // a record launch's per-pixel hit counts between its passes, beside ws.acc (rtx_device.h: launch_trace_records); allocated
    // by the first record launch of a scene with more than one ray per pixel, never by a byte launch
    DeviceBuffer ws_record_hits;
    // ray queries, ray shading and views (rtx_query.hip, rtx_shade.hip, rtx_view.hip): device copies of the host entry points' arrays, the
    // regrouping pass's (key, ray number) buffers and the sort's temporary storage; none shared with the render workspace
    DeviceBuffer q_first, q_second, q_out;
    struct { DeviceBuffer keys, keys_sorted, index, index_sorted, temp; } q_sort;
    // rtx_*_lit (rtx_light.hip): the points of the most recent lit call's light, made on that call's stream ahead of its
    // view or shade kernel; rtx_render_view_rows_lit (rtx_tour.hip) adds the tour and the boxes of that light.  One owner
    // (reserve_light, light_launch), one guard: `used` (kUsesLight)
    struct {
        DeviceBuffer points, tour, boxes;
        Event used;
    } lit;
    // rtx_render_view_mean (rtx_accum.hip): the seeded table of the frame in flight — made by rtxr::samples_kernel on the
    // call's stream, never the scene's `samples` — and that frame's records, which the add kernel reads behind the view
    // kernel.  The frame's light points go where a lit call's go (lit.points).  One guard: `used` (kUsesMean)
    struct {
        DeviceBuffer table, records;
        Event used;
    } mean;
    // rtx_scene_pose (rtx_pose.hip): the host tables (rtx::PoseTables, uploaded with the first pose), the host variant's
    // copies of the caller's arrays, and the one pose this device holds, as a geometry: posed primitive and shading
    // records, the refitted stream, — host variant with a reference tree — that tree's stream, the plane records of the
    // pose's global triangles (rtx_planes.hip, made with the pose) and the primary rays' stream of the most recent posed
    // view's eye, which posed and unposed views of one eye do not share.  One guard: `used` (kUsesPose)
    struct {
        DeviceBuffer tri_of, ranges, order;
        bool tables = false;
        DeviceBuffer v, rank;
        DeviceGeometry geo;
        bool valid = false;
        Event used;
        // rtx_scene_pose_rebuilt (rtx_rebuild.hip): the rebuilt stream's host tables (rtx::RebuildTables, uploaded with the
        // first rebuilt pose: link and info as node records, ranges, order), the sort's buffers and the permutation.
        // rebuilt: the pose that stands is a rebuilt one (geo.n_nodes is then the rebuilt stream's count)
        struct {
            DeviceBuffer nodes, ranges, order;
            bool tables = false;
            DeviceBuffer keys, keys_sorted, index, perm, temp;
        } b;
        bool rebuilt = false;
        // rtx_scene_pose_prims (rtx_prims.hip): the host table (rtx::PoseTables::sphere_of, uploaded with the first such
        // pose), the host variant's copies of the caller's sphere and colour arrays, and the overlay the pose or rebuild
        // kernels of such a pose read in place of the uploaded records.  No other pose touches any of them.
        struct {
            DeviceBuffer sphere_of;
            bool tables = false;
            DeviceBuffer spheres, rgb, sphere_rgb;
            DeviceBuffer tris, shade;
        } m;
        // rtx_scene_pose_moved (rtx_move.hip): the scene's rest geometry and its tables (rtx::PreparedScene::rest_*, uploaded
        // with the first such pose) and the host variant's copies of the caller's moves, groups and radius factors.  The
        // move kernel writes `v` and `m.spheres` above — the buffers the host poses copy a caller's arrays into — and the
        // pose reads them from there as it reads those copies.  ran: they hold what the move kernel last wrote
        // (rtx_debug_moved_prims); a host pose that copies into them takes it away.
        struct {
            DeviceBuffer rest_v, rest_spheres, tri_vec, sphere_vec;
            bool tables = false;
            DeviceBuffer moves, group, radius_scale;
            bool ran = false;
        } f;
        // rtx_scene_pose_skinned (rtx_skin.hip): this device's copy of the scene's skin (RtxScene::skin), uploaded with the
        // first skinned pose after a bind.  generation: the bind it is a copy of (0: none yet).  The skin kernel reads the
        // rest geometry of `f` and writes where the move kernel writes, f.ran included.
        struct {
            DeviceBuffer bones, weights, sphere_bone;
            uint64_t generation = 0;
        } k;
    } pose;
private:
    ~DeviceState() = default;
    friend struct ReleaseOnDevice;
};

// The one place a DeviceState and everything it owns is released — after an upload that failed half way and in
// rtx_scene_destroy — with its own device current and the library's stream drained, whatever the caller had current.
// A device that cannot be made current is skipped: the state is abandoned (leaked) on purpose, since its owners would
// otherwise hand their handles to whatever device happens to be current.
struct ReleaseOnDevice {
    void operator()(DeviceState *st) const
    {
        DeviceGuard g(st->device);
        if (g.status() != hipSuccess) return;
        if (st->stream) (void)hipStreamSynchronize(st->stream);
        delete st;
    }
};

// a scene's place for one device: the lock outlives the state, which a failed upload takes away (the next call starts anew)
struct DeviceSlot {
    std::mutex mu;
    std::unique_ptr<DeviceState, ReleaseOnDevice> st;
};

// The one rule for the library-owned buffer groups an event guards.  A call states the groups it uses — the regrouping
// buffers (q_sort), the light buffers (lit), the pose (pose: its geometry, aimed stream included), the scratch table and records
// of a mean call (mean) — as a set of these bits.
// A call that uses them on the library's stream (the host bodies, the rtx_debug_* read-backs, rtx_scene_pose) waits for
// all of them first: wait_for_uses.  A device-resident call marks all of them behind its kernels on the caller's stream:
// mark_uses.  A new guarded group is one bit, one event and one line in each of the two.
enum : unsigned { kUsesSort = 1u, kUsesLight = 2u, kUsesPose = 4u, kUsesMean = 8u };

int wait_for_uses(DeviceState &st, unsigned uses)
{
    if (uses & kUsesSort) RTX_TRY(wait_for(st.q_sorted, st.stream));
    if (uses & kUsesLight) RTX_TRY(wait_for(st.lit.used, st.stream));
    if (uses & kUsesPose) RTX_TRY(wait_for(st.pose.used, st.stream));
    if (uses & kUsesMean) RTX_TRY(wait_for(st.mean.used, st.stream));
    return RTX_OK;
}

int mark_uses(DeviceState &st, unsigned uses, hipStream_t callers)
{
    if (uses & kUsesSort) RTX_TRY(mark_busy(st.q_sorted, callers));
    if (uses & kUsesLight) RTX_TRY(mark_busy(st.lit.used, callers));
    if (uses & kUsesPose) RTX_TRY(mark_busy(st.pose.used, callers));
    if (uses & kUsesMean) RTX_TRY(mark_busy(st.mean.used, callers));
    return RTX_OK;
}

double wall_ms()
{
    using namespace std::chrono;
    return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

}  // namespace

struct RtxScene {
    rtx::PreparedScene prep;
    std::mutex mu;
    rtx::PoseTables pose_tables;     // made by the first call that poses (pose_tables_of), under mu
    bool pose_tables_made = false;
    rtx::RebuildTables rebuild_tables;   // made by the first call that asks for a rebuilt pose (rebuild_tables_of), under mu
    bool rebuild_tables_made = false;
    rtx::Skin skin;                  // rtx_scene_skin, which is not re-entrant per handle: read without a lock
    std::map<int, DeviceSlot> dev;
    // rtx_debug_probe_split: which tiles the scheduling pass treats as long (0: the prediction), and how many workgroups of
    // the long list the scene's most recent pipeline launch was handed
    std::atomic<uint32_t> split_mode{0u}, last_long{0u};
};

namespace {

int device_count_quiet()
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n < 0 ? 0 : n;
}

int get_slot(RtxScene *scene, int device, DeviceSlot **out)
{
    if (device < 0 || device >= device_count_quiet()) return RTX_ERR_NO_DEVICE;
    std::lock_guard<std::mutex> lk(scene->mu);
    *out = &scene->dev[device];
    return RTX_OK;
}

// caller holds slot.mu
int ensure_state(DeviceSlot &slot, int device)
{
    if (!slot.st) slot.st.reset(new (std::nothrow) DeviceState(device));
    return slot.st ? RTX_OK : RTX_ERR_OOM;
}

// pad_bytes of zeros follow the data (the node stream carries one sentinel record)
template <class T>
int upload_vec(DeviceBuffer &dst, const std::vector<T> &v, size_t pad_bytes = 0)
{
    const size_t bytes = v.size() * sizeof(T);
    const int rc = dst.reserve(bytes + pad_bytes ? bytes + pad_bytes : 16);
    if (rc != RTX_OK) return rc;
    if (bytes) RTX_HIP(hipMemcpy(dst.as<void>(), v.data(), bytes, hipMemcpyHostToDevice));
    if (pad_bytes) RTX_HIP(hipMemset(dst.as<char>() + bytes, 0, pad_bytes));
    return RTX_OK;
}

// librtx.so runs one pipeline.  Only the ablation build (librtx_ablation.so, -DRTX_ABLATION=1: A/B tools and the
// variant-equality test) lets RTX_VARIANT pick another one, read once per process.
uint32_t kernel_variant()
{
#if RTX_ABLATION
    static const uint32_t v = [] {
        const char *e = std::getenv("RTX_VARIANT");
        return e ? static_cast<uint32_t>(std::atoi(e)) & rtx::kVariantMask : rtx::kDefaultVariant;
    }();
    return v;
#else
    return rtx::kDefaultVariant;
#endif
}

// The scene's sample table and what the scene derives from it, on the device: the table — a caller's by a copy, a seeded one
// made in place by rtxr::samples_kernel from its seed, nothing of the table's size copied — and the small light arrays
// (points, tour, boxes).  Synchronous, on the null stream: the host arrays outlive the copies and the table stands when
// this returns.  The buffers grow only.  Where earlier launches may still read the table it replaces, the caller waits for
// the device first (ensure_uploaded).  The margin and n_samples travel in every call's argument block (device_scene), read
// from the scene.
int table_upload(const rtx::PreparedScene &p, DeviceState &st)
{
    st.table_generation = ~0ull;         // until every piece stands
    if (p.seeded) {
        RTX_TRY(st.samples.reserve(std::max<size_t>(static_cast<size_t>(p.n_samples) * sizeof(float2), 16u)));
        RTX_HIP(rtxr::launch_samples(p.sample_seed, p.n_samples, st.samples.as<float2>(), nullptr));
        RTX_HIP(hipStreamSynchronize(nullptr));
    } else {
        RTX_TRY(upload_vec(st.samples, p.samples));
    }
    RTX_TRY(upload_vec(st.lights, p.light_points));
    RTX_TRY(upload_vec(st.light_tour, p.light_tour));
    RTX_TRY(upload_vec(st.light_boxes, p.light_boxes));
    st.table_generation = p.table_generation;
    return RTX_OK;
}

// the uploads of ensure_uploaded; may stop half way
int upload_all(RtxScene *scene, DeviceState &st)
{
    const rtx::PreparedScene &p = scene->prep;
    int rc;
    const float inflate = p.cull_delta;   // the culling planes move outwards: rtx_traverse.hpp, box_mask
    DeviceGeometry &g = st.geo;
    if ((rc = upload_vec(g.nodes, rtx::nodes_in_device_order(p.nodes, inflate), sizeof(rtx::NodeRec))) != RTX_OK) return rc;
    if (!p.primary_nodes.empty() &&
        (rc = upload_vec(st.primary_nodes, rtx::nodes_in_device_order(p.primary_nodes, inflate), sizeof(rtx::NodeRec))) != RTX_OK) return rc;
    if (!p.ref_nodes.empty() &&
        (rc = upload_vec(g.ref_nodes, rtx::nodes_in_device_order(p.ref_nodes), sizeof(rtx::NodeRec))) != RTX_OK) return rc;
    g.n_nodes = static_cast<uint32_t>(p.nodes.size());
    g.n_ref_nodes = static_cast<uint32_t>(p.ref_nodes.size());
    // one spare record of zeros behind the primitive records (no walk requests the record after the one it tests any more)
    if ((rc = upload_vec(g.tris, p.tris, sizeof(rtx::TriRec))) != RTX_OK) return rc;
    if ((rc = upload_vec(g.shade, p.shade)) != RTX_OK) return rc;
    if ((rc = table_upload(p, st)) != RTX_OK) return rc;
    if (!p.global_planes.empty() && (rc = upload_vec(g.planes, p.global_planes)) != RTX_OK) return rc;
    if (!p.long_tiles.empty()) {
        std::vector<uint32_t> words(p.long_tiles);
        words.insert(words.end(), p.long_bits.begin(), p.long_bits.end());
        if ((rc = upload_vec(st.long_words, words)) != RTX_OK) return rc;
    }
    if ((rc = st.thr.reserve(sizeof(p.gamma_thr))) != RTX_OK) return rc;
    RTX_HIP(hipMemcpy(st.thr.as<void>(), p.gamma_thr, sizeof(p.gamma_thr), hipMemcpyHostToDevice));
    if ((rc = st.d_counters.reserve(rtx::kNumCounters * sizeof(unsigned long long))) != RTX_OK) return rc;
    RTX_HIP(hipStreamCreateWithFlags(st.stream.put(), hipStreamNonBlocking));
    RTX_HIP(hipEventCreate(st.ev0.put()));
    RTX_HIP(hipEventCreate(st.ev1.put()));
    for (auto &slot : st.ring)
        for (Event &e : slot) RTX_HIP(hipEventCreate(e.put()));
    st.uploaded = true;
    return RTX_OK;
}

// Caller holds slot.mu, with a state in the slot.  An upload that fails half way takes the state out of the slot, and
// with it everything allocated so far: nothing leaks, and the next call starts with uploaded == false.
// A device whose table is not the scene's (rtx_scene_resample, rtx_scene_reseed) catches up here, in the first call of any
// kind after the replacement and before that call enqueues anything: it waits for the device — a launch on any stream, the
// caller's included, may still read the table, and rtx_render_view_device is tied to no stream the library knows — and
// uploads as an upload does.  Geometry, pose, skin and aimed streams are not touched.  A catch-up that fails is a failed upload.
int ensure_uploaded(RtxScene *scene, DeviceSlot &slot)
{
    int rc = RTX_OK;
    if (!slot.st->uploaded) {
        rc = upload_all(scene, *slot.st);
    } else if (slot.st->table_generation != scene->prep.table_generation) {
        rc = hip_rc(hipDeviceSynchronize());
        if (rc == RTX_OK) rc = table_upload(scene->prep, *slot.st);
    }
    if (rc != RTX_OK) slot.st.reset();
    return rc;
}

// The one way into an entry point that works on a device: the scene's slot for it, the slot's lock and a state in the
// slot; from kCurrent on the device made current (the caller's comes back on scope exit), with kUploaded the scene's
// uploads.  After rc == RTX_OK state() is good until a call that is handed the slot (launch_on) fails: a failed upload
// takes the state out of the slot.
class Entry {
public:
    enum Need { kLocked, kCurrent, kUploaded };
    Entry(RtxScene *scene, int device, Need need)
    {
        if ((rc = get_slot(scene, device, &slot)) != RTX_OK) return;
        lock_ = std::unique_lock<std::mutex>(slot->mu);
        if ((rc = ensure_state(*slot, device)) != RTX_OK) return;
        if (need >= kCurrent && (rc = make_current()) != RTX_OK) return;
        if (need >= kUploaded) rc = ensure_uploaded(scene, *slot);
    }
    int make_current() { return hip_rc(guard_.set(slot->st->device)); }
    DeviceState &state() const { return *slot->st; }
    int rc = RTX_ERR_INTERNAL;
    DeviceSlot *slot = nullptr;
private:
    std::unique_lock<std::mutex> lock_;
    DeviceGuard guard_;
};

// Which geometry a call walks: the uploaded scene's, or (posed) the pose's.  The one place that answers a posed call on
// a device that holds no pose: RTX_ERR_BAD_ARG.  The primitive count and the number of global triangles hold for both; the
// node count is the geometry's own (a rebuilt pose's tree has another one).
int geometry_of(DeviceState &st, bool posed, DeviceGeometry **out)
{
    *out = &st.geo;
    if (!posed) return RTX_OK;
    if (!st.pose.valid) return RTX_ERR_BAD_ARG;
    *out = &st.pose.geo;
    return RTX_OK;
}

// The launchers' argument block over geometry `g` of the device.  primary_nodes is the scene's own eye's stream over the
// uploaded nodes; only the pipeline reads it, and a pipeline view puts its aimed stream there (view_rows_launch).
rtx::DeviceScene device_scene(const RtxScene *scene, const DeviceState &st, const DeviceGeometry &g)
{
    const rtx::PreparedScene &p = scene->prep;
    rtx::DeviceScene S;
    S.nodes = g.nodes.as<const rtx::NodeRec>();
    S.primary_nodes = st.primary_nodes.capacity() ? st.primary_nodes.as<const rtx::NodeRec>() : st.geo.nodes.as<const rtx::NodeRec>();
    S.light_tour = st.light_tour.as<const float>();
    S.n_wide = 0u;
    S.ref_nodes = g.ref_nodes.as<const rtx::NodeRec>();
    S.n_ref_nodes = g.n_ref_nodes;
    S.tris = g.tris.as<const rtx::TriRec>();
    S.shade = g.shade.as<const rtx::ShadeRec>();
    S.samples = st.samples.as<const float2>();
    S.light_points = st.lights.as<const float>();
    S.planes = g.planes.as<const rtx::TriRec>();
    S.gamma_thr = st.thr.as<const float>();
    S.light_boxes = st.light_boxes.as<const float>();
    S.shaft_delta = p.shaft_delta;
    S.n_nodes = g.n_nodes;
    S.n_samples = p.n_samples;
    S.width = p.width;
    S.height = p.height;
    S.nb_ray = p.nb_ray;
    S.nb_light = p.nb_light_sample;
    S.n_spheres = p.n_spheres;
    S.n_global = p.n_global;
    std::memcpy(S.eye, p.eye, 12);
    std::memcpy(S.cu, p.cam_u, 12);
    std::memcpy(S.cv, p.cam_v, 12);
    std::memcpy(S.cw, p.cam_w, 12);
    S.distance = p.distance;
    S.cut_max_nodes = rtx::kCutMaxNodes;
    S.n_prims = static_cast<uint32_t>(p.tris.size());
    S.j1_mode = 0u;
#if RTX_ABLATION   // librtx_ablation.so only: one scene with and without per-tile cuts (tests/test_gpu_pipeline.py)
    if (const char *e = std::getenv("RTX_CUT_MAX_NODES")) S.cut_max_nodes = static_cast<uint32_t>(std::strtoul(e, nullptr, 10));
    if (S.cut_max_nodes > rtx::kCutEndMask) S.cut_max_nodes = rtx::kCutEndMask;     // (a cut stream's record holds a 26-bit position)
    // ... and the north_star's LDS / reduction design as measurable variants (rtx_j1_ablation.hpp); modes 2, 3: triangles only
    if (const char *e = std::getenv("RTX_J1")) {
        const uint32_t m = static_cast<uint32_t>(std::strtoul(e, nullptr, 10));
        if (m == 1u || ((m == 2u || m == 3u) && p.n_spheres == 0u)) S.j1_mode = m;
    }
#endif
    return S;
}

// sizes the workspace of the streamed pipeline for a launch and gives its argument block; *used = false: the variant has none
int reserve_stream_ws(DeviceState &st, const rtx::DeviceScene &S, const rtx::TileSpec &ts, rtx::StreamWorkspace *ws, bool *used)
{
    *used = (kernel_variant() & (rtx::kVariantStream | rtx::kVariantProbe)) != 0u;
    if (!*used) return RTX_OK;
    const rtx::StreamWorkspaceBytes need = rtx::stream_workspace_bytes(S, ts, kernel_variant());
    const int rc = reserve_all({{st.ws.hits, need.hits}, {st.ws.pix_slot, need.pix_slot}, {st.ws.tiles, need.tiles},
                                {st.ws.chunks, need.chunks}, {st.ws.results, need.results}, {st.ws.acc, need.acc},
                                {st.ws.ctr, need.ctr}, {st.ws.buckets, need.buckets}, {st.ws.cut, need.cut}});
    if (rc != RTX_OK) return rc;
    st.last_tiles = need.tiles / sizeof(rtx::TileDesc);
    *ws = rtx::StreamWorkspace{st.ws.hits.as<rtx::HitRec>(), st.ws.pix_slot.as<uint32_t>(), st.ws.tiles.as<rtx::TileDesc>(),
                               st.ws.chunks.as<uint2>(), st.ws.results.as<float>(), st.ws.acc.as<float>(),
                               st.ws.ctr.as<uint32_t>(), st.ws.buckets.as<uint32_t>(), st.ws.cut.as<rtx::CutEntry>()};
    return RTX_OK;
}

uint32_t tiles_rows(uint32_t height, uint32_t first_tile, uint32_t tile_stride, uint32_t tile_rows)
{
    if (!tile_rows || !tile_stride) return 0;
    uint64_t rows = 0;
    for (uint64_t t = first_tile; t * tile_rows < height; t += tile_stride) {
        const uint64_t r0 = t * tile_rows;
        rows += (height - r0 < tile_rows) ? (height - r0) : tile_rows;
    }
    return static_cast<uint32_t>(rows);
}

// The one mapping from a counter block to RtxStats.  Rendering and shading: primary_rays = pixels * nb_ray and
// nb_light_sample shadow rays per hit; the ray queries: their n rays and none.
void fill_stats(RtxStats *s, uint64_t primary_rays, uint32_t shadow_rays_per_hit, const unsigned long long *c,
                double kernel_ms, double total_ms)
{
    std::memset(s, 0, sizeof *s);
    s->primary_rays = primary_rays;
    s->primary_hits = c[0];
    s->shadow_rays = c[0] * shadow_rays_per_hit;
    s->rays = s->primary_rays + s->shadow_rays;
    s->box_tests = c[1];
    s->tri_tests = c[2];
    s->wave_node_visits = c[3];
    s->wave_tri_visits = c[4];
    s->redo_tiles = c[5];
    s->kernel_ms = kernel_ms;
    s->total_ms = total_ms;
}

// The bracket of a host call that times and counts on the library's stream (stats == NULL: neither).  In the call's order:
// the wall clock starts with the object; empty() answers a call without work; begin() goes on the stream once the call's
// buffers stand and whatever it copies in is enqueued, end() behind its kernels; the call enqueues its copies back, and
// gather() waits for all of it and fills the statistics.  Caller holds the slot's lock and has the device current.
struct Timed {
    explicit Timed(RtxStats *s) : stats(s) {}
    RtxStats *const stats;
    const double t0 = wall_ms();
    unsigned long long *counters(const DeviceState &st) const { return stats ? st.d_counters.as<unsigned long long>() : nullptr; }
    int empty() const
    {
        const unsigned long long none[rtx::kNumCounters] = {0};
        if (stats) fill_stats(stats, 0, 0, none, 0.0, wall_ms() - t0);
        return RTX_OK;
    }
    int begin(const DeviceState &st) const
    {
        if (stats) RTX_HIP(hipMemsetAsync(counters(st), 0, rtx::kNumCounters * sizeof(unsigned long long), st.stream));
        RTX_HIP(hipEventRecord(st.ev0, st.stream));
        return RTX_OK;
    }
    int end(const DeviceState &st) const { return hip_rc(hipEventRecord(st.ev1, st.stream)); }
    int gather(const DeviceState &st, uint64_t primary_rays, uint32_t shadow_rays_per_hit) const
    {
        unsigned long long c[rtx::kNumCounters] = {0};
        if (stats) RTX_HIP(hipMemcpyAsync(c, counters(st), sizeof c, hipMemcpyDeviceToHost, st.stream));
        RTX_HIP(hipStreamSynchronize(st.stream));
        if (!stats) return RTX_OK;
        float ms = 0.0f;
        RTX_HIP(hipEventElapsedTime(&ms, st.ev0, st.ev1));
        fill_stats(stats, primary_rays, shadow_rays_per_hit, c, ms, wall_ms() - t0);
        return RTX_OK;
    }
};

// The one render launch, on `stream`: the redo queue and the streamed pipeline's workspace sized, `before()` (what the
// caller puts on the stream once the buffers stand), the kernels, the launch's slot of the timing ring.  The per-tile
// profile (d_wave_prof, ablation build) is the fused kernel's: no workspace, no slot.  Caller holds the slot's lock and
// has the device current and the scene uploaded.  The redo queue is library-owned per device: launches on one device
// must be ordered on one stream.
// split: the long list of the scene's own view (probe_split_of), or none.
// d_shade: NULL, or where the launch writes RtxPixelShade records in place of d_out's bytes (the record forms of the kernels
// that store a pixel: the two-pass pipeline's alone, without a profile or a list).
// mask (with d_shade): NULL, or the tile states and the rule behind which the record launch schedules its tiles
// (rtx_device.h: launch_trace_records_masked).
struct TileMask {
    const void *d_tiles;
    RtxAdaptRule rule;
};
template <class Before>
int render_launch(DeviceState &st, const rtx::DeviceScene &S, const rtx::TileSpec &ts, uint8_t *d_out,
                  unsigned long long *d_counters, unsigned long long *d_wave_prof, hipStream_t stream, Before before,
                  const rtx::ProbeSplit &split = rtx::ProbeSplit{nullptr, 0u, 0u, 0u}, void *d_shade = nullptr,
                  const TileMask *mask = nullptr)
{
    int rc;
    const size_t redo_cap = st.d_redo.capacity(), buckets_cap = st.ws.buckets.capacity();
    if ((rc = st.d_redo.reserve(rtx::trace_redo_bytes(S, ts))) != RTX_OK) return rc;
    rtx::StreamWorkspace ws{};
    bool use_ws = false;
    if (!d_wave_prof && (rc = reserve_stream_ws(st, S, ts, &ws, &use_ws)) != RTX_OK) return rc;
    if (d_shade) {
        if (d_wave_prof || !use_ws || !(kernel_variant() & rtx::kVariantProbe)) return RTX_ERR_UNSUPPORTED;
        const size_t hits_bytes = rtx::trace_record_hits_bytes(S, ts);
        if (hits_bytes && (rc = st.ws_record_hits.reserve(hits_bytes)) != RTX_OK) return rc;
    }
    if ((rc = before()) != RTX_OK) return rc;
    const Event *slot = st.ring[st.launches % RTX_TIMING_RING];
    hipEvent_t phases[3] = {slot[0], slot[1], slot[2]};
    const bool two_pass = use_ws && (kernel_variant() & rtx::kVariantProbe) != 0u && ts.local_rows != 0u;
    if (two_pass && (!st.launch_words_ready || st.d_redo.capacity() != redo_cap || st.ws.buckets.capacity() != buckets_cap)) {
        RTX_HIP(rtx::zero_launch_words(st.d_redo.as<uint32_t>(), ws, stream));
        st.words_launches = st.words_passes = 0;
    }
    if (ts.local_rows) st.launch_words_ready = false;     // until this launch is known to have gone out whole
    if (d_shade && mask)
        RTX_HIP(rtx::launch_trace_records_masked(S, ts, d_shade, S.nb_ray > 1u ? st.ws_record_hits.as<uint8_t>() : nullptr,
                                                 st.d_redo.as<uint32_t>(), &ws, d_counters, kernel_variant(), stream, phases,
                                                 st.words_launches, st.words_passes, mask->d_tiles, mask->rule));
    else if (d_shade)
        RTX_HIP(rtx::launch_trace_records(S, ts, d_shade, S.nb_ray > 1u ? st.ws_record_hits.as<uint8_t>() : nullptr, st.d_redo.as<uint32_t>(),
                                          &ws, d_counters, kernel_variant(), stream, phases, st.words_launches, st.words_passes));
    else
        RTX_HIP(rtx::launch_trace_shade(S, ts, d_out, st.d_redo.as<uint32_t>(), use_ws ? &ws : nullptr, d_counters, d_wave_prof,
                                        kernel_variant(), stream, d_wave_prof ? nullptr : phases, st.words_launches, st.words_passes, split));
    if (two_pass) {
        st.launch_words_ready = true;
        ++st.words_launches;
        st.words_passes += S.nb_ray;
    }
    if (!d_wave_prof && ts.local_rows) ++st.launches;
    return RTX_OK;
}

// The long list a launch of the scene's own view over its uploaded geometry is handed (rtx_render_rows, rtx_render_frame,
// rtx_render_tiles_device), by the scene's mode: the prediction, none, or every tile of the frame.  None as well where
// the launcher would drop it (probe_split_applies): the whole-stream form, a share whose tiles are not the frame's, a launch of
// more than 65,536 tiles.  The view calls and the
// posed ones never ask: their stream is aimed from another eye, their boxes are not the ones the prediction weighed.
// Records what it answers (rtx_debug_probe_split).  Caller holds the slot's lock and has the device current and the scene
// uploaded.
int probe_split_of(RtxScene *scene, DeviceState &st, const rtx::DeviceScene &S, const rtx::TileSpec &ts, rtx::ProbeSplit *out)
{
    *out = rtx::ProbeSplit{nullptr, 0u, 0u, 0u};
    scene->last_long = 0u;
    const uint32_t mode = scene->split_mode;
    if (mode == 1u || !rtx::probe_split_applies(S, ts)) return RTX_OK;
    if (mode == 2u) {
        if (!st.n_long_all) {
            const uint32_t n = ((S.width + 7u) / 8u) * ((S.height + 7u) / 8u);
            std::vector<uint32_t> words(n + (n + 31u) / 32u, 0xFFFFFFFFu);
            for (uint32_t t = 0; t < n; ++t) words[t] = t;
            RTX_TRY(upload_vec(st.long_all, words));
            st.n_long_all = n;
        }
        const uint32_t tx = (S.width + 7u) / 8u, ty = (S.height + 7u) / 8u;
        if (tx - 1u <= 0xFFFFu && ty - 1u <= 0xFFFFu)
            *out = rtx::ProbeSplit{st.long_all.as<const uint32_t>(), st.n_long_all, (tx - 1u) << 16, (ty - 1u) << 16};
    } else if (!scene->prep.long_tiles.empty()) {
        const std::vector<uint32_t> &tiles = scene->prep.long_tiles;
        rtx::ProbeSplit listed{st.long_words.as<const uint32_t>(), static_cast<uint32_t>(tiles.size()), 0u, 0u};
        if (rtx::probe_split_ranges(tiles.data(), listed.n_long, (S.width + 7u) / 8u, &listed)) *out = listed;
    }
    scene->last_long = out->n_long;
    return RTX_OK;
}

// launch one device's share into its d_out, between timed's begin() and end(); caller holds slot.mu, with a state in the
// slot, and has the device current
int launch_on(RtxScene *scene, DeviceSlot &slot, const rtx::TileSpec &ts, const Timed &timed)
{
    RTX_TRY(ensure_uploaded(scene, slot));
    DeviceState &st = *slot.st;
    const size_t bytes = static_cast<size_t>(ts.local_rows) * scene->prep.width * 3u;
    RTX_TRY(st.d_out.reserve(bytes ? bytes : 16));
    const rtx::DeviceScene S = device_scene(scene, st, st.geo);
    rtx::ProbeSplit split;
    RTX_TRY(probe_split_of(scene, st, S, ts, &split));
    RTX_TRY(render_launch(st, S, ts, st.d_out.as<uint8_t>(), timed.counters(st), nullptr, st.stream,
                          [&] { return timed.begin(st); }, split));
    return timed.end(st);
}

// ---- ray batches: the queries (rtx_query.hip), shading (rtx_shade.hip) and views (rtx_view.hip) -------------------------

// first record of the tree proper: behind the root and the leaf of the global triangles when there are any
uint32_t tree_root(const rtx::PreparedScene &p, size_t n_nodes)
{
    return (p.n_global != 0u && n_nodes > 2u) ? 2u : 0u;
}
uint32_t tree_root(const rtx::PreparedScene &p) { return tree_root(p, p.nodes.size()); }

// The multiply-based culling of the walks is proven for origins whose coordinates stay within the magnitude behind
// cull_delta (scene_prep.cpp): the bound the ray-batch kernels are handed, and the one a pipeline view's eye is held to.
float origin_bound(const RtxScene *scene) { return scene->prep.cull_delta * 0x1p19f; }

// The box the regrouping keys quantise origins in: the tree proper's root (beside the global triangles — the ground is
// as large as the scene and would leave the mesh a handful of cells), else the stream's root.
rtxq::KeyBox query_key_box(const rtx::PreparedScene &p)
{
    rtxq::KeyBox box{};
    if (p.nodes.empty()) return box;
    const rtx::NodeRec &root = p.nodes[tree_root(p)];
    for (int a = 0; a < 3; ++a) {
        const float extent = root.bmax[a] - root.bmin[a];
        const float scale = static_cast<float>(1u << rtxq::kMortonBitsPerAxis) / extent;
        box.lo[a] = root.bmin[a];
        box.scale[a] = (extent > 0.0f && scale > 0.0f && scale < 0x1p100f) ? scale : 0.0f;   // (false for a NaN)
    }
    return box;
}

// sizes the regrouping pass's buffers for n entries and gives their argument block; caller holds the slot's lock and has
// the device current
int reserve_query_sort(DeviceState &st, uint32_t n, rtxq::SortBuffers *sort)
{
    const size_t words = static_cast<size_t>(n) * sizeof(uint32_t);
    size_t temp = 0;
    RTX_HIP(rtxq::sort_temp_bytes(n, &temp));
    const int rc = reserve_all({{st.q_sort.keys, words}, {st.q_sort.keys_sorted, words}, {st.q_sort.index, words},
                                {st.q_sort.index_sorted, words}, {st.q_sort.temp, temp ? temp : 16}});
    if (rc != RTX_OK) return rc;
    *sort = rtxq::SortBuffers{st.q_sort.keys.as<uint32_t>(), st.q_sort.keys_sorted.as<uint32_t>(), st.q_sort.index.as<uint32_t>(),
                              st.q_sort.index_sorted.as<uint32_t>(), st.q_sort.temp.as<void>(), st.q_sort.temp.capacity()};
    return RTX_OK;
}

static_assert(sizeof(RtxRayHit) == 32, "closest_kernel writes a hit as two 16-byte words");
static_assert(sizeof(RtxPixelShade) == 16, "shade_kernel writes a pixel as one 16-byte word");
static_assert(sizeof(RtxView) == sizeof(rtxv::ViewBlock) && alignof(RtxView) == 4, "view_kernel is handed an RtxView");
constexpr uint32_t kQueryFlags = RTX_RAYS_KEEP_ORDER | RTX_RAYS_FORCE_REGROUP;

// n_pixels * nb_ray, or 0 when it is beyond what one batch may hold
uint32_t shade_ray_count(const RtxScene *scene, uint32_t n_pixels)
{
    const uint64_t n = static_cast<uint64_t>(n_pixels) * scene->prep.nb_ray;
    return n <= rtxq::kMaxRays ? static_cast<uint32_t>(n) : 0u;
}

// what a family's launcher is handed: the scene, the regrouping pass's box, bound and buffers (NULL: the caller's order),
// the two input arrays (a view has none: its kernel makes the rays), the view (or NULL), the outputs, the counters (or
// NULL), all on the device, and the stream
constexpr int kBatchOuts = 3;
struct BatchArgs {
    rtx::DeviceScene S;
    uint32_t n;
    const float *first, *second;
    const RtxView *view;
    rtxq::KeyBox box;
    float origin_bound;
    const rtxq::SortBuffers *sort;
    void *out[kBatchOuts];
    unsigned long long *counters;
    hipStream_t stream;
};

template <bool Occlusion>
hipError_t launch_queried(const BatchArgs &a)
{
    return rtxq::launch_query(a.S, Occlusion, a.n, a.first, a.second, a.box, a.origin_bound, a.sort, a.out[0], a.counters, a.stream);
}

hipError_t launch_shaded(const BatchArgs &a)
{
    return rtxs::launch_shade(a.S, a.n, a.first, a.second, a.box, a.origin_bound, a.sort, a.out[0], a.out[1], a.counters, a.stream);
}

// a view's outputs in Batch::out_bytes' order: the 16-byte records first, so that they stay aligned in the library's buffer
enum { kViewShade, kViewHits, kViewRgb };

hipError_t launch_viewed(const BatchArgs &a)
{
    rtxv::ViewBlock v;
    std::memcpy(&v, a.view, sizeof v);
    return rtxv::launch_view(a.S, v, a.origin_bound, a.out[kViewRgb], a.out[kViewShade], a.out[kViewHits], a.counters, a.stream);
}

// What a lit call takes from its RtxLight: the triangle and the sample count, the scene's for 0 (lit_of)
struct Lit {
    rtxl::LightTriangle tri;
    uint32_t count;
};

// What differs between rtx_trace_rays, rtx_occluded_rays, rtx_shade_rays and rtx_render_view (and their _device and _lit
// twins), checked by them.
struct Batch {
    uint32_t n;                    // entries the launcher works on and the regrouping pass sorts: rays, or pixels of nb_ray rays
    uint32_t n_rays;               // rays in each of the two input arrays (a view: rays its kernel makes)
    uint32_t flags;
    size_t out_bytes[kBatchOuts];  // the output segments, one behind the other in the library's device buffer (a segment
                                   // of 16-byte records follows multiples of 16 only: it stays aligned); 0: none
    uint32_t shadow_rays_per_hit;  // RtxStats
    hipError_t (*launch)(const BatchArgs &);
    const RtxView *view;           // rtx_render_view: the caller's, read while the call runs; else NULL
    const Lit *lit;                // the lit twins: the call's light (shadow_rays_per_hit is its count); else NULL
    bool posed;                    // the posed twins: the device's pose in place of the uploaded geometry (geometry_of)
};

// the guarded groups a call with this light (or NULL) and this switch uses, the regrouping buffers aside
unsigned uses_of(const Lit *lit, bool posed)
{
    unsigned uses = 0u;
    if (lit) uses |= kUsesLight;
    if (posed) uses |= kUsesPose;
    return uses;
}

bool batch_regroups(const Batch &b)
{
    if (b.flags & RTX_RAYS_KEEP_ORDER) return false;
    return b.n >= rtxq::kRegroupMinRays || (b.flags & RTX_RAYS_FORCE_REGROUP) != 0u;
}

// A call's light on the device.  The view and shade kernels read its points and count (rtx_shade_pixel.hpp); the render
// pipeline's kernels also walk its tour and boxes and test shafts with its margin (rtx_kernel.hip) — `walk`, here and below.
// The buffers are library-owned per device and grow only.  reserve_light sizes them before the call's kernels that read them
// are on a stream; growing one waits for the device first, since an earlier launch may still read it.  Caller holds the
// slot's lock and has the device current and the scene uploaded.
int reserve_light(const RtxScene *scene, DeviceState &st, const Lit &lit, bool walk)
{
    const size_t rays = scene->prep.nb_ray, n = rays * lit.count;
    const size_t points = std::max<size_t>(n * 3u * sizeof(float), 16u);
    const size_t tour = walk ? std::max<size_t>(n * 4u * sizeof(float), 16u) : 0u;
    const size_t boxes = walk ? std::max<size_t>(rays * 6u * sizeof(float), 16u) : 0u;
    if (st.lit.points.capacity() >= points && st.lit.tour.capacity() >= tour && st.lit.boxes.capacity() >= boxes) return RTX_OK;
    RTX_HIP(hipDeviceSynchronize());
    return reserve_all({{st.lit.points, points}, {st.lit.tour, tour}, {st.lit.boxes, boxes}});
}

// the light kernels on `stream`, after reserve_light: the points; walk: their tour and their boxes too
// (table / n_pairs: NULL — the scene's table — or a mean call's frame table)
int light_launch(const RtxScene *scene, DeviceState &st, const Lit &lit, bool walk, hipStream_t stream, const float2 *table = nullptr,
                 uint32_t n_pairs = 0u)
{
    const rtx::PreparedScene &p = scene->prep;
    if (lit.count == 0u) return RTX_OK;      // (the scene's own count is 0 then: no kernel reads a point)
    RTX_HIP(rtxl::launch_light_points(table ? table : st.samples.as<const float2>(), table ? n_pairs : p.n_samples, lit.tri, p.nb_ray,
                                      lit.count, st.lit.points.as<float>(), stream));
    if (!walk) return RTX_OK;
    RTX_HIP(rtxt::launch_tour(st.lit.points.as<const float>(), p.nb_ray, lit.count, st.lit.tour.as<float>(), stream));
    RTX_HIP(rtxt::launch_light_boxes(st.lit.points.as<const float>(), p.nb_ray, lit.count, st.lit.boxes.as<float>(), stream));
    return RTX_OK;
}

// ... and the fields of the call's copy of the scene's argument block that the kernels read of the light; the pipeline's
// workspace and the LDS of its launch are sized by S.nb_light.  shaft_delta: lit_rows_margin's (walk only)
void light_swap(const DeviceState &st, const Lit &lit, bool walk, float shaft_delta, rtx::DeviceScene *S)
{
    if (lit.count == 0u) return;
    S->light_points = st.lit.points.as<const float>();
    S->nb_light = lit.count;
    if (!walk) return;
    S->light_tour = st.lit.tour.as<const float>();
    S->light_boxes = st.lit.boxes.as<const float>();
    S->shaft_delta = shaft_delta;
}

bool light_is_finite(const Lit &lit)
{
    for (float x : lit.tri.v)
        if (!std::isfinite(x)) return false;
    return true;
}

// What the render pipeline reads of a call's light beside its points, as the host states it: per primary ray and batch the
// tour as sample indices (rtx_scene_light_order's form), the boxes, and the shaft margin, PreparedScene::shaft_delta's fold
// over this light's boxes.  Each output may be NULL.  O(nb_ray * count) for the margin alone; the tour costs what
// light_tour_order_f32 costs.  May throw std::bad_alloc.
// samples: the table the points are made over — the scene's as it stands, or a mean call's frame (seeded: scene_prep.cpp's
// light_walk_statement reads the nb_ray * count entries the points read and makes no table)
void light_walk_on_host(const rtx::PreparedScene &p, const Lit &lit, const rtx::SampleSource &samples, uint32_t *order, float *boxes,
                        float *shaft_delta)
{
    rtx::light_walk_statement(p, lit.tri.v, lit.count, samples, order, boxes, shaft_delta);
}
void light_walk_on_host(const rtx::PreparedScene &p, const Lit &lit, uint32_t *order, float *boxes, float *shaft_delta)
{
    light_walk_on_host(p, lit, rtx::sample_source(p), order, boxes, shaft_delta);
}

// The checks a lit pipeline call adds on the host, before a device is looked for, and the margin of its shaft test: the
// vertices finite, and the margin finite — prepare_scene's own rule, so that a pipeline call accepts exactly the lights
// rtx_scene_create would accept.  A count of 0 (the scene's own is 0 and so is the light's): nothing is swapped.
int lit_rows_margin(const RtxScene *scene, const Lit &lit, float *shaft_delta)
{
    if (!light_is_finite(lit)) return RTX_ERR_UNSUPPORTED;
    *shaft_delta = scene->prep.shaft_delta;
    if (lit.count == 0u) return RTX_OK;
    try {
        light_walk_on_host(scene->prep, lit, nullptr, nullptr, shaft_delta);
    } catch (...) {
        return RTX_ERR_OOM;
    }
    return std::isfinite(*shaft_delta) ? RTX_OK : RTX_ERR_UNSUPPORTED;
}

// ---- posing (rtx_scene_pose; the kernels: rtx_pose.hip) --------------------------------------------------------------------

// the scene's host tables, made once; may throw std::bad_alloc
const rtx::PoseTables &pose_tables_of(RtxScene *scene)
{
    std::lock_guard<std::mutex> lk(scene->mu);
    if (!scene->pose_tables_made) {
        rtx::pose_tables(scene->prep, scene->pose_tables);
        scene->pose_tables_made = true;
    }
    return scene->pose_tables;
}

uint32_t posed_triangles(const RtxScene *scene) { return scene->prep.n_tris - scene->prep.n_spheres; }

// the rebuilt stream's host tables, made once; may throw std::bad_alloc
const rtx::RebuildTables &rebuild_tables_of(RtxScene *scene)
{
    std::lock_guard<std::mutex> lk(scene->mu);
    if (!scene->rebuild_tables_made) {
        rtx::rebuild_tables(scene->prep, scene->rebuild_tables);
        scene->rebuild_tables_made = true;
    }
    return scene->rebuild_tables;
}

// What a pose states (the ten rtx_scene_pose* entry points), as host pointers for a host call and as device pointers for a
// device-resident one: the vertices (NULL: the scene has no triangle, or the device makes them), the tie ranks (NULL:
// none), what it states beside the vertices, the moves the device makes the vertices and the spheres from (n_moves == 0:
// none), the skin that blends them (NULL: every primitive follows its group's move) and whether the tree is rebuilt.
// spheres: the pose states spheres — ov.spheres, or the device's own output for a moved pose of a scene that has some.
struct PoseCall {
    const float *v = nullptr;
    const uint32_t *tie_rank = nullptr;
    rtx::PrimsOverlay ov;
    rtx::PoseMoves moves;
    const rtx::Skin *skin = nullptr;
    bool rebuilt = false;
    bool spheres = false;
    bool moved() const { return moves.n_moves != 0u; }
    bool overlaid() const { return spheres || ov.rgb || ov.sphere_rgb; }      // the overlay kernel runs, its buffers are used
};

// a pose that states its vertices alone
PoseCall vertices_alone(const float *v, const uint32_t *tie_rank, bool rebuilt) { return {v, tie_rank, {}, {}, nullptr, rebuilt, false}; }

// The one rule for growing the pose's buffers, library-owned per device and grow-only: when one of `list` is too small the
// pose is marked invalid, the device is waited for — an earlier launch may still read what is freed — and all are reserved;
// otherwise nothing happens.  moved_list: the list is the moved pose's own, and what the move kernel last wrote
// (rtx_debug_moved_prims) goes with it; no other growth takes that away.
int grow_pose(DeviceState &st, std::initializer_list<Sized> list, bool moved_list)
{
    if (std::all_of(list.begin(), list.end(), [](const Sized &s) { return s.buffer.capacity() >= s.bytes; })) return RTX_OK;
    st.pose.valid = false;
    if (moved_list) st.pose.f.ran = false;
    RTX_HIP(hipDeviceSynchronize());
    return reserve_all(list);
}

// Every pose's buffers (grow_pose), and the tables' upload with the first pose.  host_copies: room for the host variant's
// copies of the vertices and the ranks.  n_ref: records of the reference tree's stream that goes beside the pose (host
// variant), or 0.  rebuilt: the node records are sized for the rebuilt stream, and the sort's buffers and the rebuilt
// stream's tables come with them (uploaded with the first rebuilt pose).  Caller holds the slot's lock and has the device
// current and the scene uploaded, here and in the three below.
int reserve_pose(RtxScene *scene, DeviceState &st, bool host_copies, size_t n_ref, bool rebuilt)
{
    const rtx::PreparedScene &p = scene->prep;
    const rtx::RebuildTables *bt = nullptr;
    try {
        if (rebuilt) bt = &rebuild_tables_of(scene);
    } catch (...) {
        return RTX_ERR_OOM;
    }
    const size_t n_prims = p.tris.size(), n_nodes = bt ? bt->nodes.size() : p.nodes.size();
    const size_t n_tree = n_prims - p.n_global;
    const size_t keys = rebuilt ? std::max<size_t>(n_tree * sizeof(uint64_t), 16u) : 0u;
    const size_t index = rebuilt ? std::max<size_t>(n_tree * sizeof(uint32_t), 16u) : 0u;
    size_t temp = 0;
    if (rebuilt) {
        RTX_HIP(rtxb::sort_temp_bytes(static_cast<uint32_t>(n_tree), &temp));
        if (temp < 16u) temp = 16u;
    }
    auto &q = st.pose;
    DeviceGeometry &g = q.geo;
    RTX_TRY(grow_pose(st, {{g.tris, (n_prims + 1u) * sizeof(rtx::TriRec)},
                           {g.shade, std::max<size_t>(n_prims * sizeof(rtx::ShadeRec), 16u)},
                           {g.nodes, (n_nodes + 1u) * sizeof(rtx::NodeDev)},
                           {g.ref_nodes, n_ref ? (n_ref + 1u) * sizeof(rtx::NodeDev) : 0u},
                           {q.v, host_copies ? std::max<size_t>(static_cast<size_t>(posed_triangles(scene)) * 9u * sizeof(float), 16u) : 0u},
                           {q.rank, host_copies ? std::max<size_t>(n_prims * sizeof(uint32_t), 16u) : 0u},
                           {g.planes, static_cast<size_t>(p.n_global) * sizeof(rtx::TriRec)},      // (no global triangle: no buffer)
                           {q.b.keys, keys}, {q.b.keys_sorted, keys}, {q.b.index, index}, {q.b.perm, index}, {q.b.temp, temp}},
                      false));
    try {
        if (!q.tables) {
            const rtx::PoseTables &t = pose_tables_of(scene);
            RTX_TRY(upload_vec(q.tri_of, t.tri_of));
            RTX_TRY(upload_vec(q.ranges, t.ranges));
            RTX_TRY(upload_vec(q.order, t.order));
            q.tables = true;
        }
        if (bt && !q.b.tables) {
            RTX_TRY(upload_vec(q.b.nodes, rtx::nodes_in_device_order(bt->nodes)));
            RTX_TRY(upload_vec(q.b.ranges, bt->ranges));
            RTX_TRY(upload_vec(q.b.order, bt->order));
            q.b.tables = true;
        }
    } catch (...) {
        return RTX_ERR_OOM;
    }
    return RTX_OK;
}

// The overlay's buffers of a pose that states spheres or colours, beside reserve_pose's: the overlay's records — the
// primitive records only where spheres are stated — and, host_copies, room for the host variant's copies of the arrays the
// call gives (the spheres' also where the device makes them); sphere_of is uploaded with the first such pose.
int reserve_prims(RtxScene *scene, DeviceState &st, bool host_copies, const PoseCall &c)
{
    const rtx::PreparedScene &p = scene->prep;
    const size_t n_prims = p.tris.size(), n_spheres = p.n_spheres, n_triangles = posed_triangles(scene);
    auto &m = st.pose.m;
    RTX_TRY(grow_pose(st, {{m.tris, c.spheres ? std::max<size_t>(n_prims * sizeof(rtx::TriRec), 16u) : 0u},
                           {m.shade, std::max<size_t>(n_prims * sizeof(rtx::ShadeRec), 16u)},
                           {m.spheres, host_copies && c.spheres ? std::max<size_t>(n_spheres * 4u * sizeof(float), 16u) : 0u},
                           {m.rgb, host_copies && c.ov.rgb ? std::max<size_t>(n_triangles * 3u * sizeof(float), 16u) : 0u},
                           {m.sphere_rgb, host_copies && c.ov.sphere_rgb ? std::max<size_t>(n_spheres * 3u * sizeof(float), 16u) : 0u}},
                      false));
    try {
        if (!m.tables) {
            RTX_TRY(upload_vec(m.sphere_of, pose_tables_of(scene).sphere_of));
            m.tables = true;
        }
    } catch (...) {
        return RTX_ERR_OOM;
    }
    return RTX_OK;
}

// The buffers of a moved pose, beside reserve_pose's: the two arrays the move kernel writes (pose.v, pose.m.spheres) and,
// host_copies, room for the host variant's copies of what `mv` gives; the rest geometry is uploaded with the first such pose.
int reserve_moves(RtxScene *scene, DeviceState &st, bool host_copies, const rtx::PoseMoves &mv)
{
    const rtx::PreparedScene &p = scene->prep;
    auto &q = st.pose;
    RTX_TRY(grow_pose(st, {{q.v, std::max<size_t>(p.rest_v0v1v2.size() * sizeof(float), 16u)},
                           {q.m.spheres, std::max<size_t>(p.rest_spheres.size() * sizeof(float), 16u)},
                           {q.f.moves, host_copies ? static_cast<size_t>(mv.n_moves) * 12u * sizeof(float) : 0u},
                           {q.f.group, host_copies && mv.group ? std::max<size_t>(p.tris.size() * sizeof(uint32_t), 16u) : 0u},
                           {q.f.radius_scale, host_copies && mv.radius_scale ? static_cast<size_t>(mv.n_moves) * sizeof(float) : 0u}},
                      true));
    if (!q.f.tables) {
        RTX_TRY(upload_vec(q.f.rest_v, p.rest_v0v1v2));
        RTX_TRY(upload_vec(q.f.rest_spheres, p.rest_spheres));
        RTX_TRY(upload_vec(q.f.tri_vec, p.rest_tri_vec));
        RTX_TRY(upload_vec(q.f.sphere_vec, p.rest_sphere_vec));
        q.f.tables = true;
    }
    return RTX_OK;
}

// This device's copy of the scene's skin (rtx_scene_pose_skinned), after reserve_moves: library-owned, grow-only, uploaded
// when the scene's generation is not the copy's.  A device-resident skinned pose may still read the copy a re-bind
// replaces, so the upload waits for the device; it happens once per bind.  No pose is touched.
int reserve_skin(RtxScene *scene, DeviceState &st)
{
    const rtx::Skin &k = scene->skin;
    auto &q = st.pose.k;
    if (q.generation == k.generation) return RTX_OK;
    RTX_HIP(hipDeviceSynchronize());
    q.generation = 0u;
    RTX_TRY(upload_vec(q.bones, k.bones));
    RTX_TRY(upload_vec(q.weights, k.weights));
    RTX_TRY(upload_vec(q.sphere_bone, k.sphere_bone));
    q.generation = k.generation;
    return RTX_OK;
}

// The pose kernels on `stream`, after the reservations; `d` is the call over device arrays, the caller's or the library's
// copies of them.  In this order: the move kernel, or with a skin the skin kernel, makes pose.v and pose.m.spheres, which
// then stand for the call's vertices and spheres; the overlay kernel restates what the call states beside the vertices, and
// the others read its records where they read the uploaded ones (nothing stated: no launch, none of its buffers touched);
// the pose kernels refit the uploaded stream or — rebuilt — the rebuild kernels and the sort make the records in sorted
// order and the refit runs alone over the rebuilt stream's tables, whose node count becomes the geometry's; the plane kernel
// runs over the posed global triangles (none: no launch).  The records behind the last one (upload_all pads the scene's
// with the same) are zeroed on the same stream.  This is the only writer of the pose's nodes, and it takes the aimed
// stream's validity away before anything is launched (AimedStream).
int pose_launch(RtxScene *scene, DeviceState &st, const PoseCall &d, hipStream_t stream)
{
    const rtx::PreparedScene &p = scene->prep;
    const bool rebuilt = d.rebuilt;
    const uint32_t n_prims = static_cast<uint32_t>(p.tris.size());
    const uint32_t n_nodes = static_cast<uint32_t>(rebuilt ? scene->rebuild_tables.nodes.size() : p.nodes.size());   // (made: reserve_pose)
    DeviceGeometry &q = st.pose.geo;
    st.pose.valid = false;
    q.aimed.valid = false;
    q.n_nodes = n_nodes;
    st.pose.rebuilt = rebuilt;
    RTX_HIP(hipMemsetAsync(q.tris.as<rtx::TriRec>() + n_prims, 0, sizeof(rtx::TriRec), stream));
    RTX_HIP(hipMemsetAsync(q.nodes.as<rtx::NodeDev>() + n_nodes, 0, sizeof(rtx::NodeDev), stream));
    const float *d_pose = d.v;
    rtx::PrimsOverlay d_ov = d.ov;
    if (d.moved()) {
        auto &f = st.pose.f;
        auto common = [&](auto &a) {
            a.rest_v = f.rest_v.as<const float>();
            a.rest_spheres = f.rest_spheres.as<const float>();
            a.n_triangles = posed_triangles(scene);
            a.n_spheres = p.n_spheres;
            a.n_moves = d.moves.n_moves;
            a.moves = d.moves.moves;
            a.radius_scale = d.moves.radius_scale;
            a.out_v = st.pose.v.as<float>();
            a.out_spheres = st.pose.m.spheres.as<float>();
        };
        f.ran = false;
        if (d.skin) {
            rtxk::SkinArgs k{};
            common(k);
            k.bones = st.pose.k.bones.as<const uint4>();
            k.weights = st.pose.k.weights.as<const float4>();
            k.sphere_bone = st.pose.k.sphere_bone.as<const uint32_t>();
            RTX_HIP(rtxk::launch_skin(k, stream));
        } else {
            rtxf::MoveArgs m{};
            common(m);
            m.tri_vec = f.tri_vec.as<const uint32_t>();
            m.sphere_vec = f.sphere_vec.as<const uint32_t>();
            m.group = d.moves.group;
            RTX_HIP(rtxf::launch_move(m, stream));
        }
        f.ran = true;
        d_pose = posed_triangles(scene) ? st.pose.v.as<const float>() : nullptr;
        d_ov.spheres = p.n_spheres ? st.pose.m.spheres.as<const float>() : nullptr;
    }
    rtxp::PoseArgs a{};
    a.tris = st.geo.tris.as<const rtx::TriRec>();
    a.shade = st.geo.shade.as<const rtx::ShadeRec>();
    if (d_ov.any()) {
        rtxm::OverlayArgs o{};
        o.tris = a.tris;
        o.shade = a.shade;
        o.tri_of = st.pose.tri_of.as<const uint32_t>();
        o.sphere_of = st.pose.m.sphere_of.as<const uint32_t>();
        o.n_prims = n_prims;
        o.spheres = d_ov.spheres;
        o.rgb = d_ov.rgb;
        o.sphere_rgb = d_ov.sphere_rgb;
        o.ov_tris = d_ov.spheres ? st.pose.m.tris.as<rtx::TriRec>() : nullptr;
        o.ov_shade = st.pose.m.shade.as<rtx::ShadeRec>();
        RTX_HIP(rtxm::launch_overlay(o, stream));
        if (o.ov_tris) a.tris = o.ov_tris;
        a.shade = o.ov_shade;
    }
    // a scene without triangles reads no vertex: the launchers still want a pointer
    if (!d_pose && posed_triangles(scene) == 0u) d_pose = reinterpret_cast<const float *>(a.tris);
    a.nodes = (rebuilt ? st.pose.b.nodes : st.geo.nodes).as<const rtx::NodeDev>();
    a.tri_of = st.pose.tri_of.as<const uint32_t>();
    a.ranges = (rebuilt ? st.pose.b.ranges : st.pose.ranges).as<const uint2>();
    a.order = (rebuilt ? st.pose.b.order : st.pose.order).as<const uint32_t>();
    a.n_prims = n_prims;
    a.n_nodes = n_nodes;
    a.n_long = rebuilt ? scene->rebuild_tables.n_long : scene->pose_tables.n_long;      // (made: reserve_pose)
    a.cull_delta = p.cull_delta;
    a.pose = d_pose;
    a.rank = d.tie_rank;
    a.out_tris = q.tris.as<rtx::TriRec>();
    a.out_shade = q.shade.as<rtx::ShadeRec>();
    a.out_nodes = q.nodes.as<rtx::NodeDev>();
    if (rebuilt) {
        rtxb::RebuildArgs r{};
        r.tris = a.tris;
        r.shade = a.shade;
        r.tri_of = a.tri_of;
        r.n_prims = n_prims;
        r.n_global = p.n_global;
        r.bound = p.scene_magnitude;
        r.scale = rtx::rebuild_key_scale(p.scene_magnitude);
        r.pose = d_pose;
        r.rank = d.tie_rank;
        r.keys = st.pose.b.keys.as<uint64_t>();
        r.keys_sorted = st.pose.b.keys_sorted.as<uint64_t>();
        r.index = st.pose.b.index.as<uint32_t>();
        r.perm = st.pose.b.perm.as<uint32_t>();
        r.temp = st.pose.b.temp.as<void>();
        r.temp_bytes = st.pose.b.temp.capacity();
        r.out_tris = a.out_tris;
        r.out_shade = a.out_shade;
        RTX_HIP(rtxb::launch_rebuild(r, stream));
        RTX_HIP(rtxp::launch_refit(a, stream));
    } else {
        RTX_HIP(rtxp::launch_pose(a, stream));
    }
    RTX_HIP(rtxg::launch_global_planes(q.tris.as<const rtx::TriRec>(), p.n_global, q.planes.as<rtx::TriRec>(), stream));
    q.n_ref_nodes = 0u;
    st.pose.valid = true;
    return RTX_OK;
}

// key + sort + kernel of one batch on `stream`, the light kernel of a lit one ahead of them; caller holds the slot's lock,
// has the device current and the scene uploaded
int batch_launch(RtxScene *scene, DeviceState &st, const Batch &b, const float *d_first, const float *d_second,
                 void *const d_out[kBatchOuts], unsigned long long *d_counters, hipStream_t stream)
{
    rtxq::SortBuffers sort{};
    const bool regroup = batch_regroups(b);
    if (regroup) RTX_TRY(reserve_query_sort(st, b.n, &sort));
    DeviceGeometry *geo;
    RTX_TRY(geometry_of(st, b.posed, &geo));
    rtx::DeviceScene S = device_scene(scene, st, *geo);
    if (b.lit) {
        RTX_TRY(reserve_light(scene, st, *b.lit, false));
        RTX_TRY(light_launch(scene, st, *b.lit, false, stream));
        light_swap(st, *b.lit, false, 0.0f, &S);
    }
    RTX_HIP(b.launch(BatchArgs{S, b.n, d_first, d_second, b.view, query_key_box(scene->prep), origin_bound(scene),
                               regroup ? &sort : nullptr, {d_out[0], d_out[1], d_out[2]}, d_counters, stream}));
    return RTX_OK;
}

// the host entry points: copy in (first, second: the two input arrays, or NULL twice), launch, copy out
int batch_host(RtxScene *scene, int device, const Batch &b, const float *first, const float *second,
               void *const (&out)[kBatchOuts], RtxStats *stats)
{
    const Timed timed(stats);
    if (b.n == 0u) return timed.empty();
    if (b.lit && !light_is_finite(*b.lit)) return RTX_ERR_UNSUPPORTED;
    Entry e(scene, device, Entry::kUploaded);
    if (e.rc != RTX_OK) return e.rc;
    DeviceState &st = e.state();
    const size_t in_bytes = first ? static_cast<size_t>(b.n_rays) * 3u * sizeof(float) : 0u;
    size_t offset[kBatchOuts + 1] = {0};
    for (int k = 0; k < kBatchOuts; ++k) offset[k + 1] = offset[k] + b.out_bytes[k];
    RTX_TRY(reserve_all({{st.q_first, in_bytes}, {st.q_second, in_bytes}, {st.q_out, offset[kBatchOuts]}}));
    void *d_out[kBatchOuts];
    for (int k = 0; k < kBatchOuts; ++k) d_out[k] = b.out_bytes[k] ? st.q_out.as<uint8_t>() + offset[k] : nullptr;
    // a device-resident call may still be sorting (waited for whether this batch regroups or not), reading its light's
    // points, or making the pose
    RTX_TRY(wait_for_uses(st, kUsesSort | uses_of(b.lit, b.posed)));
    if (in_bytes) {
        RTX_HIP(hipMemcpyAsync(st.q_first.as<void>(), first, in_bytes, hipMemcpyHostToDevice, st.stream));
        RTX_HIP(hipMemcpyAsync(st.q_second.as<void>(), second, in_bytes, hipMemcpyHostToDevice, st.stream));
    }
    RTX_TRY(timed.begin(st));
    const int rc = batch_launch(scene, st, b, st.q_first.as<float>(), st.q_second.as<float>(), d_out, timed.counters(st), st.stream);
    if (rc != RTX_OK) {
        (void)hipStreamSynchronize(st.stream);      // the copies above read the caller's arrays
        return rc;
    }
    RTX_TRY(timed.end(st));
    for (int k = 0; k < kBatchOuts; ++k)
        if (b.out_bytes[k]) RTX_HIP(hipMemcpyAsync(out[k], d_out[k], b.out_bytes[k], hipMemcpyDeviceToHost, st.stream));
    return timed.gather(st, b.n_rays, b.shadow_rays_per_hit);
}

// the device-resident entry points: the caller's arrays, the caller's stream, nothing waited for
int batch_device(RtxScene *scene, int device, const Batch &b, const void *d_first, const void *d_second,
                 void *const (&d_out)[kBatchOuts], void *stream)
{
    if ((reinterpret_cast<uintptr_t>(d_first) | reinterpret_cast<uintptr_t>(d_second)) & 3u) return RTX_ERR_BAD_ARG;
    if (b.n == 0u) return RTX_OK;
    if (b.lit && !light_is_finite(*b.lit)) return RTX_ERR_UNSUPPORTED;
    Entry e(scene, device, Entry::kUploaded);
    if (e.rc != RTX_OK) return e.rc;
    DeviceState &st = e.state();
    RTX_TRY(batch_launch(scene, st, b, static_cast<const float *>(d_first), static_cast<const float *>(d_second), d_out, nullptr,
                         static_cast<hipStream_t>(stream)));
    const unsigned sorts = batch_regroups(b) ? kUsesSort : 0u;
    return mark_uses(st, sorts | uses_of(b.lit, b.posed), static_cast<hipStream_t>(stream));
}

// the argument checks a family's host and device-resident entry points share
bool query_args_ok(const RtxScene *scene, const void *first, const void *second, const void *out, uint32_t flags, uint32_t n_rays)
{
    return scene && first && second && out && !(flags & ~kQueryFlags) && n_rays <= rtxq::kMaxRays;
}

bool shade_args_ok(const RtxScene *scene, const void *first, const void *second, const void *out, uint32_t flags, uint32_t n_pixels)
{
    if (!scene || !first || !second || !out || (flags & ~kQueryFlags)) return false;
    return n_pixels == 0u || shade_ray_count(scene, n_pixels) != 0u;
}

Batch query_batch(bool occlusion, uint32_t n_rays, uint32_t flags, bool posed)
{
    return Batch{n_rays, n_rays, flags, {static_cast<size_t>(n_rays) * (occlusion ? 1u : sizeof(RtxRayHit)), 0u, 0u}, 0u,
                 occlusion ? launch_queried<true> : launch_queried<false>, nullptr, nullptr, posed};
}

// Caller has checked n_pixels (shade_args_ok).  lit, here and below: NULL for the scene's light, else the call's (lit_of):
// the light kernel runs ahead of the batch's kernel, and the statistics count the light's samples per hit.
Batch shade_batch(const RtxScene *scene, uint32_t n_pixels, uint32_t flags, const Lit *lit, bool posed, bool want_hits)
{
    const uint32_t n_rays = shade_ray_count(scene, n_pixels);
    return Batch{n_pixels, n_rays, flags,
                 {static_cast<size_t>(n_pixels) * sizeof(RtxPixelShade), want_hits ? static_cast<size_t>(n_rays) * sizeof(RtxRayHit) : 0u, 0u},
                 lit ? lit->count : scene->prep.nb_light_sample, launch_shaded, nullptr, lit, posed};
}

// a frame has pixels, and fewer than 2^31 of them
bool frame_ok(const RtxView *v)
{
    return v->width != 0u && v->height != 0u && static_cast<uint64_t>(v->width) * v->height < (1ull << 31);
}

// the argument checks rtx_render_view and its twins share (`rgb`, `shade`, `hits`: the three outputs)
bool view_args_ok(const RtxScene *scene, const RtxView *v, const void *rgb, const void *shade, const void *hits)
{
    if (!scene || !v || (!rgb && !shade && !hits) || !frame_ok(v)) return false;
    if (static_cast<uint64_t>(v->x0) + v->nx > v->width || static_cast<uint64_t>(v->y0) + v->ny > v->height) return false;
    return static_cast<uint64_t>(v->nx) * v->ny * scene->prep.nb_ray <= rtxv::kMaxRays;     // (nx * ny < 2^31)
}

// caller has checked the view (view_args_ok); the rays are made tile by tile: no regrouping pass
Batch view_batch(const RtxScene *scene, const RtxView *v, const Lit *lit, bool posed, const void *rgb, const void *shade,
                 const void *hits)
{
    const uint32_t n_pixels = v->nx * v->ny, n_rays = n_pixels * scene->prep.nb_ray;
    Batch b{n_pixels, n_rays, RTX_RAYS_KEEP_ORDER, {0u, 0u, 0u}, lit ? lit->count : scene->prep.nb_light_sample, launch_viewed, v, lit,
            posed};
    b.out_bytes[kViewShade] = shade ? static_cast<size_t>(n_pixels) * sizeof(RtxPixelShade) : 0u;
    b.out_bytes[kViewHits] = hits ? static_cast<size_t>(n_rays) * sizeof(RtxRayHit) : 0u;
    b.out_bytes[kViewRgb] = rgb ? static_cast<size_t>(n_pixels) * 3u : 0u;
    return b;
}

// a device-resident call writes 16-byte records (RtxPixelShade, RtxRayHit) through these; NULL: an output not asked for
bool aligned16(const void *a, const void *b = nullptr)
{
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15u) == 0u;
}

static_assert(sizeof(RtxLight) == 40 && alignof(RtxLight) == 4 && offsetof(RtxLight, nb_light_sample) == sizeof(rtxl::LightTriangle),
              "the light kernel is handed the first 36 bytes of an RtxLight");

// The argument checks the lit entry points add to their twins': a light, and at most kMaxCallLightPoints points.  *out: the
// call's copy of the light (the caller's may change while the call runs), the count the scene's for 0.
bool lit_of(const RtxScene *scene, const RtxLight *light, Lit *out)
{
    if (!scene || !light) return false;
    std::memcpy(out->tri.v, light->v0, 12);
    std::memcpy(out->tri.v + 3, light->v1, 12);
    std::memcpy(out->tri.v + 6, light->v2, 12);
    out->count = light->nb_light_sample ? light->nb_light_sample : scene->prep.nb_light_sample;
    return static_cast<uint64_t>(scene->prep.nb_ray) * out->count <= rtx::kMaxCallLightPoints;
}

// The light of a call that takes an RtxLight, checked before everything else of the call (lit_of's rules).  kRequired (the
// _lit entry points): a NULL light fails.  kOptional (the _posed ones): a NULL light is the scene's own, lit == NULL.
// !ok: the call answers RTX_ERR_BAD_ARG.
struct CallLight {
    enum Need { kRequired, kOptional };
    CallLight(const RtxScene *scene, const RtxLight *light, Need need)
        : ok((!light && need == kOptional) || lit_of(scene, light, &copy)), lit(light && ok ? &copy : nullptr) {}
    Lit copy;
    const bool ok;
    const Lit *const lit;
};

// The bodies of rtx_render_view and rtx_shade_rays, each with its _lit twin's light as an argument.  A view's outputs in
// Batch::out_bytes' order: {shade, hits, rgb}.
static_assert(kViewShade == 0 && kViewHits == 1 && kViewRgb == 2, "view_host and view_device list a view's outputs in this order");
int view_host(RtxScene *scene, int device, const RtxView *view, const Lit *lit, bool posed, uint8_t *rgb, RtxPixelShade *shade,
              RtxRayHit *hits, RtxStats *stats)
{
    if (!view_args_ok(scene, view, rgb, shade, hits)) return RTX_ERR_BAD_ARG;
    return batch_host(scene, device, view_batch(scene, view, lit, posed, rgb, shade, hits), nullptr, nullptr, {shade, hits, rgb}, stats);
}

int view_device(RtxScene *scene, int device, const RtxView *view, const Lit *lit, bool posed, void *d_rgb, void *d_shade, void *d_hits,
                void *stream)
{
    if (!view_args_ok(scene, view, d_rgb, d_shade, d_hits) || !aligned16(d_shade, d_hits)) return RTX_ERR_BAD_ARG;
    return batch_device(scene, device, view_batch(scene, view, lit, posed, d_rgb, d_shade, d_hits), nullptr, nullptr,
                        {d_shade, d_hits, d_rgb}, stream);
}

int shade_host(RtxScene *scene, int device, uint32_t n_pixels, const float *origins, const float *directions, uint32_t flags,
               const Lit *lit, bool posed, RtxPixelShade *shade, RtxRayHit *hits, RtxStats *stats)
{
    if (!shade_args_ok(scene, origins, directions, shade, flags, n_pixels)) return RTX_ERR_BAD_ARG;
    return batch_host(scene, device, shade_batch(scene, n_pixels, flags, lit, posed, hits != nullptr), origins, directions,
                      {shade, hits, nullptr}, stats);
}

int shade_device(RtxScene *scene, int device, uint32_t n_pixels, const void *d_origins, const void *d_directions, uint32_t flags,
                 const Lit *lit, bool posed, void *d_shade, void *d_hits, void *stream)
{
    if (!shade_args_ok(scene, d_origins, d_directions, d_shade, flags, n_pixels) || !aligned16(d_shade, d_hits)) return RTX_ERR_BAD_ARG;
    return batch_device(scene, device, shade_batch(scene, n_pixels, flags, lit, posed, d_hits != nullptr), d_origins, d_directions,
                        {d_shade, d_hits, nullptr}, stream);
}

// ---- the mean of N frames: what a call is and what it reserves (the one path: below, behind the pipeline's view launch) ------

// What a mean call is beside its view: the light (the scene's own as a Lit when the caller gave none: every frame's points
// are made over that frame's table), whether the caller gave it (the twin's finiteness check is for a given light), the
// geometry switch, the seeds and the table's length.
struct MeanCall {
    Lit lit;
    bool given;
    bool posed;
    const uint64_t *seeds;
    uint32_t n_frames, n_pairs;
};

// the argument checks every mean call shares, the twin's (CallLight, view_args_ok: `out` stands for its outputs) among them
bool mean_args_ok(const RtxScene *scene, const RtxView *view, const RtxLight *light, uint32_t flags, const uint64_t *seeds,
                  uint32_t n_frames, uint32_t n_pairs, const void *out, MeanCall *call)
{
    if (!scene || !seeds || n_frames == 0u || n_frames > rtx::kMaxMeanFrames || n_pairs == 0u || (flags & ~RTX_MEAN_POSED)) return false;
    RtxLight own;
    if (!light && rtx_scene_light(scene, &own) != RTX_OK) return false;
    if (!lit_of(scene, light ? light : &own, &call->lit)) return false;
    if (!view_args_ok(scene, view, nullptr, out, nullptr)) return false;
    call->given = light != nullptr;
    call->posed = (flags & RTX_MEAN_POSED) != 0u;
    call->seeds = seeds;
    call->n_frames = n_frames;
    call->n_pairs = n_pairs;
    return true;
}

// The scratch table and records of a mean call, library-owned per device, grow only; growing one waits for the device
// first, as reserve_light does: an earlier launch may still read it.
int reserve_mean(DeviceState &st, uint32_t n_pairs, uint32_t n_pixels)
{
    const size_t table = std::max<size_t>(static_cast<size_t>(n_pairs) * sizeof(float2), 16u);
    const size_t records = static_cast<size_t>(n_pixels) * sizeof(RtxPixelShade);
    if (st.mean.table.capacity() >= table && st.mean.records.capacity() >= records) return RTX_OK;
    RTX_HIP(hipDeviceSynchronize());
    return reserve_all({{st.mean.table, table}, {st.mean.records, records}});
}

// the guarded groups every mean call uses (the pipeline's tour and boxes are the light's: kUsesLight)
unsigned mean_uses(const MeanCall &call) { return kUsesLight | kUsesMean | (call.posed ? kUsesPose : 0u); }

// ---- any view through the render pipeline (rtx_render_view_rows; the aim kernels: rtx_aim.hip) ------------------------------

// the pipeline's walks start at the eye: origin_bound holds for it.  A NaN fails it.
bool eye_in_pipeline_range(const RtxScene *scene, const float eye[3])
{
    const float bound = origin_bound(scene);
    for (int k = 0; k < 3; ++k)
        if (!(std::fabs(eye[k]) <= bound)) return false;
    return true;
}

// the argument checks rtx_render_view_rows and its twins share: rtx_render_view's, and full width
bool view_rows_args_ok(const RtxScene *scene, const RtxView *v, const void *out)
{
    if (!scene || !v || !out || !frame_ok(v)) return false;
    if (v->x0 != 0u || v->nx != v->width) return false;
    return static_cast<uint64_t>(v->y0) + v->ny <= v->height;
}

// The stream the view's primary rays walk over geometry `g`, on `stream`: g's shadow stream when the scene has no primary
// stream of its own (nothing is aimed then), else g's aimed buffer, the aim kernels run first unless it stands for this eye
// on this stream.  Caller holds the slot's lock and has the device current and the scene uploaded; reserve_aimed() comes
// first.  Each geometry has its own aimed buffer, so that posed and unposed views of one eye alternate without aiming
// either again, and neither is handed the other's stream.
int reserve_aimed(const RtxScene *scene, DeviceGeometry &g)
{
    if (scene->prep.primary_nodes.empty()) return RTX_OK;
    AimedStream &a = g.aimed;
    const size_t n = g.n_nodes;
    const size_t had = a.nodes.capacity();
    const int rc = reserve_all({{a.nodes, (n + 1u) * sizeof(rtx::NodeDev)}, {a.links, n * sizeof(rtxa::AimLink)}});
    if (rc != RTX_OK || a.nodes.capacity() != had) a.valid = false;
    return rc;
}

const rtx::NodeRec *aimed_stream(const RtxScene *scene, const DeviceGeometry &g)
{
    return (scene->prep.primary_nodes.empty() ? g.nodes : g.aimed.nodes).as<const rtx::NodeRec>();
}

int aim_at(const RtxScene *scene, DeviceGeometry &g, const float eye[3], hipStream_t stream)
{
    const rtx::PreparedScene &p = scene->prep;
    if (p.primary_nodes.empty()) return RTX_OK;
    AimedStream &a = g.aimed;
    if (a.valid && a.on == stream && std::memcmp(a.eye, eye, 12) == 0) return RTX_OK;
    a.valid = false;
    const uint32_t n = g.n_nodes;
    RTX_HIP(hipMemsetAsync(a.nodes.as<rtx::NodeDev>() + n, 0, sizeof(rtx::NodeDev), stream));      // the sentinel
    RTX_HIP(rtxa::launch_aim(g.nodes.as<const rtx::NodeDev>(), n, tree_root(p, n), eye, a.links.as<rtxa::AimLink>(),
                             a.nodes.as<rtx::NodeDev>(), stream));
    std::memcpy(a.eye, eye, 12);
    a.on = stream;
    a.valid = true;
    return RTX_OK;
}

// rtx_render_rows / rtx_render_tiles_device for a view: device_scene() over geometry `g` (geometry_of) with the view's
// frame and camera and the stream aimed over g's nodes, rows [y0, y0 + ny) as one share.  `before`: as render_launch's; the
// aim kernels follow it on the stream.  lit: NULL, or the call's light with its margin (lit_rows_margin): the light kernels
// follow the aim kernels, and the pipeline's kernels are handed that light's five fields.  Whichever geometry it is, no
// field of the block is added or moved, and the kernels are the same.  So is the shaft margin: it is folded from the bound M
// every posed coordinate respects, not from the geometry's extent.
// table / n_pairs: NULL, or a table on the device that stands in for the scene's: the light kernels and the pipeline's read
// it.  Whoever hands one in makes it on the stream in `before`.
// mask (with d_shade): NULL, or the tile mask of the record launch (render_launch).
template <class Before>
int view_rows_launch(RtxScene *scene, DeviceState &st, DeviceGeometry &g, const RtxView &v, uint8_t *d_out,
                     unsigned long long *d_counters, hipStream_t stream, Before before, const Lit *lit, float shaft_delta,
                     void *d_shade = nullptr, const float2 *table = nullptr, uint32_t n_pairs = 0u, const TileMask *mask = nullptr)
{
    RTX_TRY(reserve_aimed(scene, g));
    if (lit) RTX_TRY(reserve_light(scene, st, *lit, true));
    rtx::DeviceScene S = device_scene(scene, st, g);
    if (lit) light_swap(st, *lit, true, shaft_delta, &S);
    if (table) {
        S.samples = table;
        S.n_samples = n_pairs;
    }
    S.width = v.width;
    S.height = v.height;
    std::memcpy(S.eye, v.eye, 12);
    std::memcpy(S.cu, v.u, 12);
    std::memcpy(S.cv, v.v, 12);
    std::memcpy(S.cw, v.w, 12);
    S.distance = v.distance;
    S.primary_nodes = aimed_stream(scene, g);
    const rtx::TileSpec ts{v.y0, v.ny, v.ny, v.ny};
    scene->last_long = 0u;      // (a view's launch is handed no long list: probe_split_of)
    return render_launch(st, S, ts, d_out, d_counters, nullptr, stream, [&]() -> int {
        RTX_TRY(before());
        RTX_TRY(aim_at(scene, g, v.eye, stream));
        return lit ? light_launch(scene, st, *lit, true, stream, table, n_pairs) : RTX_OK;
    }, rtx::ProbeSplit{nullptr, 0u, 0u, 0u}, d_shade, mask);
}

// What a pipeline view with rows is checked for on the host, before a device is looked for: the eye in range, and with a
// light of its own lit_rows_margin's rules; *shaft_delta: that light's margin.
int view_rows_supported(const RtxScene *scene, const RtxView *view, const Lit *lit, float *shaft_delta)
{
    if (!eye_in_pipeline_range(scene, view->eye)) return RTX_ERR_UNSUPPORTED;
    return lit ? lit_rows_margin(scene, *lit, shaft_delta) : RTX_OK;
}

// ---- the mean of N frames, one path: a renderer and the sums as arguments (rtx_render_view_mean, rtx_render_view_rows_mean,
// ---- rtx_render_view_adaptive and their _device twins; the kernels: rtx_accum.hip, rtx_adapt.hip) -------------------------------

// The shaft margin of every frame of a mean call, on the host, before a device is looked for: frame k's light points are made
// over the seeded table (seeds[k], n_pairs), and the margin is shaft_delta_of over their boxes — light_walk_on_host's, which
// reads the nb_ray * count entries the points read and makes no table.  n_frames * nb_ray * count point statements.
// RTX_ERR_UNSUPPORTED when a frame's margin is not finite (prepare_scene's rule, per frame).
int rows_mean_margins(const RtxScene *scene, const MeanCall &call, std::vector<float> *margins)
{
    try {
        margins->assign(call.n_frames, scene->prep.shaft_delta);
        if (call.lit.count == 0u) return RTX_OK;
        for (uint32_t k = 0; k < call.n_frames; ++k) {
            light_walk_on_host(scene->prep, call.lit, rtx::SampleSource{nullptr, call.seeds[k], call.n_pairs}, nullptr, nullptr,
                               &(*margins)[k]);
            if (!std::isfinite((*margins)[k])) return RTX_ERR_UNSUPPORTED;
        }
    } catch (...) {
        return RTX_ERR_OOM;
    }
    return RTX_OK;
}

// What renders a frame of a mean call into the scratch records: the view kernel as it is; the masked view kernel, which
// skips the tiles the sums' rule has stopped (it reads the sums' tile states: moments only); or the pipeline's record
// launch (full width, a shaft margin per frame: rows_mean_margins); or that launch behind the sums' tile states (a first
// frame: the unmasked one), which does not schedule the stopped tiles.
enum class Renderer { kView, kMasked, kRows, kRowsMasked };
bool through_pipeline(Renderer renderer) { return renderer == Renderer::kRows || renderer == Renderer::kRowsMasked; }

// What a frame's records are summed into and resolved from.  rule == NULL: the plain sum (rtx_accum.hip), d_state one
// 16-byte accumulator per pixel.  Else the moments (rtx_adapt.hip): d_state 32-byte moments, d_tiles a state per 8 x 8 tile;
// resume: no frame is a first one (both hold an earlier call's state).  A host call lays state_bytes() out with place().
struct Sums {
    const RtxAdaptRule *rule = nullptr;
    bool resume = false;
    void *d_state = nullptr, *d_tiles = nullptr;

    size_t tiles_bytes(const RtxView &v) const { return rule ? static_cast<size_t>(rtxe::tile_count(v.nx, v.ny)) * sizeof(RtxTileState) : 0u; }
    size_t pixels_bytes(const RtxView &v) const { return static_cast<size_t>(v.nx) * v.ny * (rule ? sizeof(RtxMomentPixel) : sizeof(RtxPixelShade)); }
    size_t state_bytes(const RtxView &v) const { return pixels_bytes(v) + ((tiles_bytes(v) + 15u) & ~static_cast<size_t>(15u)); }
    void place(const RtxView &v, uint8_t *d)
    {
        d_state = d;
        d_tiles = rule ? d + pixels_bytes(v) : nullptr;
    }
    hipError_t add(const RtxView &v, const void *records, bool first, hipStream_t stream) const
    {
        return rule ? rtxe::launch_moment_add(v.nx, v.ny, records, d_state, d_tiles, first, *rule, stream)
                    : rtxc::launch_accum_add(v.nx * v.ny, records, d_state, first, stream);
    }
    hipError_t resolve(const float *thr, const RtxView &v, uint32_t n_frames, void *d_rgb, void *d_shade, hipStream_t stream) const
    {
        return rule ? rtxe::launch_moment_resolve(thr, v.nx * v.ny, d_state, d_rgb, d_shade, stream)
                    : rtxc::launch_accum_resolve(thr, v.nx * v.ny, d_state, n_frames, d_rgb, d_shade, stream);
    }
    // What a host call copies out beside records and bytes, and *pixel_frames, the pixels it rendered over all frames (its
    // statistics' primary rays, per ray of a pixel).  The plain sum: nothing, every pixel of every frame.  The moments: the
    // tile states, for the caller or for the count (`count`: read back whether asked for or not, and the stream is waited
    // for), and a tile's pixels inside the rectangle times its frames.
    int copy_out(const RtxView &v, uint32_t n_frames, RtxTileState *tiles, bool count, hipStream_t stream, uint64_t *pixel_frames) const
    {
        *pixel_frames = static_cast<uint64_t>(n_frames) * v.nx * v.ny;
        if (!rule || (!tiles && !count)) return RTX_OK;
        const size_t n_tiles = tiles_bytes(v) / sizeof(RtxTileState);
        std::vector<RtxTileState> own(tiles ? 0u : n_tiles);
        if (!tiles) tiles = own.data();
        RTX_HIP(hipMemcpyAsync(tiles, d_tiles, tiles_bytes(v), hipMemcpyDeviceToHost, stream));
        if (!count) return RTX_OK;
        RTX_HIP(hipStreamSynchronize(stream));
        *pixel_frames = 0;
        const uint32_t tiles_x = (v.nx + 7u) / 8u;
        for (size_t t = 0; t < n_tiles; ++t) {
            const uint32_t x = static_cast<uint32_t>(t % tiles_x) * 8u, y = static_cast<uint32_t>(t / tiles_x) * 8u;
            *pixel_frames += static_cast<uint64_t>(std::min(8u, v.nx - x)) * std::min(8u, v.ny - y) * tiles[t].frames;
        }
        return RTX_OK;
    }
};

// Every mean call's chain on `stream`, nothing waited for between frames.  Per frame: the frame's table from its seed into
// the scratch table, the light's arrays over that table (the points; for the pipeline their tour and boxes too), the
// renderer into the scratch records — its argument block's table, table length and light fields are what differs from the
// twin's — and the add.  Then the resolve, where an output is asked for.  The pipeline launch puts the first two on the
// stream itself, once its buffers stand; its aim kernels run once, there is one eye.  The scene's own table and light
// arrays are neither read nor written.  margins: the pipeline's renderers only.  Caller holds the slot's lock and has the device current and
// the scene uploaded; the rectangle is not empty.
int frames_launch(RtxScene *scene, DeviceState &st, const RtxView &view, const MeanCall &call, Renderer renderer, const float *margins,
                  const Sums &sums, void *d_rgb, void *d_shade, unsigned long long *d_counters, hipStream_t stream)
{
    const bool rows = through_pipeline(renderer);
    DeviceGeometry *geo;
    RTX_TRY(geometry_of(st, call.posed, &geo));
    RTX_TRY(reserve_mean(st, call.n_pairs, view.nx * view.ny));
    RTX_TRY(reserve_light(scene, st, call.lit, rows));
    const float2 *table = st.mean.table.as<const float2>();
    void *records = st.mean.records.as<void>();
    rtx::DeviceScene S = device_scene(scene, st, *geo);      // (the view kernels': the pipeline launch makes its own)
    S.samples = table;
    S.n_samples = call.n_pairs;
    light_swap(st, call.lit, false, 0.0f, &S);
    rtxv::ViewBlock v;
    std::memcpy(&v, &view, sizeof v);
    for (uint32_t k = 0; k < call.n_frames; ++k) {
        const bool first = k == 0u && !sums.resume;
        const auto seed = [&] { return hip_rc(rtxr::launch_samples(call.seeds[k], call.n_pairs, st.mean.table.as<float2>(), stream)); };
        if (rows) {
            const TileMask mask{sums.d_tiles, sums.rule ? *sums.rule : RtxAdaptRule{1u, 0.0f}};
            RTX_TRY(view_rows_launch(scene, st, *geo, view, nullptr, d_counters, stream, seed, &call.lit, margins[k], records, table,
                                     call.n_pairs, renderer == Renderer::kRowsMasked && !first ? &mask : nullptr));
        } else {
            RTX_TRY(seed());
            RTX_TRY(light_launch(scene, st, call.lit, false, stream, table, call.n_pairs));
            RTX_HIP(renderer == Renderer::kMasked
                        ? rtxe::launch_view_masked(S, v, origin_bound(scene), records, d_counters, sums.d_tiles, first, *sums.rule, stream)
                        : rtxv::launch_view(S, v, origin_bound(scene), nullptr, records, nullptr, d_counters, stream));
        }
        RTX_HIP(sums.add(view, records, first, stream));
    }
    if (d_rgb || d_shade) RTX_HIP(sums.resolve(st.thr.as<const float>(), view, call.n_frames, d_rgb, d_shade, stream));
    return RTX_OK;
}

// What a mean call is refused for on the host, before a device is looked for, in each family's own order (the host tests pin
// them).  The view kernels: a given light that is not finite (the scene's own is not checked).  The pipeline: not full
// width, even for an eye out of range; then the eye, the light, given or not, and the frames' margins.  An empty rectangle
// answers RTX_OK ahead of everything but the width: the caller returns its empty answer.
int frames_refused(const RtxScene *scene, const RtxView *view, const MeanCall &call, Renderer renderer, std::vector<float> *margins)
{
    const bool rows = through_pipeline(renderer);
    if (rows && (view->x0 != 0u || view->nx != view->width)) return RTX_ERR_BAD_ARG;
    if (view->nx * view->ny == 0u) return RTX_OK;
    if (rows && !eye_in_pipeline_range(scene, view->eye)) return RTX_ERR_UNSUPPORTED;
    if ((rows || call.given) && !light_is_finite(call.lit)) return RTX_ERR_UNSUPPORTED;
    return rows ? rows_mean_margins(scene, call, margins) : RTX_OK;
}

// the host entry points: the sums' state and the outputs in the library's output buffer, one behind the other (every part
// a multiple of 16 bytes but the last), launch on the library's stream, copy out.  A host call never resumes.
int frames_host(RtxScene *scene, int device, const RtxView *view, const MeanCall &call, Renderer renderer, const RtxAdaptRule *rule,
                uint8_t *rgb, RtxPixelShade *shade, RtxTileState *tiles, RtxStats *stats)
{
    const Timed timed(stats);
    std::vector<float> margins;
    RTX_TRY(frames_refused(scene, view, call, renderer, &margins));
    if (view->nx * view->ny == 0u) return timed.empty();
    Entry e(scene, device, Entry::kUploaded);
    if (e.rc != RTX_OK) return e.rc;
    DeviceState &st = e.state();
    const RtxView v = *view;                 // (the caller's may change while the call runs)
    Sums sums{rule};
    const size_t state = sums.state_bytes(v);
    const size_t shade_bytes = shade ? static_cast<size_t>(v.nx) * v.ny * sizeof(RtxPixelShade) : 0u;
    const size_t rgb_bytes = rgb ? static_cast<size_t>(v.nx) * v.ny * 3u : 0u;
    RTX_TRY(st.q_out.reserve(state + shade_bytes + rgb_bytes));
    uint8_t *d_shade = shade ? st.q_out.as<uint8_t>() + state : nullptr, *d_rgb = rgb ? st.q_out.as<uint8_t>() + state + shade_bytes : nullptr;
    sums.place(v, st.q_out.as<uint8_t>());
    RTX_TRY(wait_for_uses(st, mean_uses(call)));
    RTX_TRY(timed.begin(st));
    RTX_TRY(frames_launch(scene, st, v, call, renderer, margins.data(), sums, d_rgb, d_shade, timed.counters(st), st.stream));
    RTX_TRY(timed.end(st));
    if (shade) RTX_HIP(hipMemcpyAsync(shade, d_shade, shade_bytes, hipMemcpyDeviceToHost, st.stream));
    if (rgb) RTX_HIP(hipMemcpyAsync(rgb, d_rgb, rgb_bytes, hipMemcpyDeviceToHost, st.stream));
    uint64_t pixel_frames = 0;
    RTX_TRY(sums.copy_out(v, call.n_frames, tiles, stats != nullptr, st.stream, &pixel_frames));
    return timed.gather(st, pixel_frames * scene->prep.nb_ray, call.lit.count);
}

// the device-resident entry points: the caller's arrays (in `sums` and d_rgb, d_shade), the caller's stream, no counters,
// nothing waited for
int frames_device(RtxScene *scene, int device, const RtxView *view, const MeanCall &call, Renderer renderer, const Sums &sums,
                  void *d_rgb, void *d_shade, void *stream)
{
    std::vector<float> margins;
    RTX_TRY(frames_refused(scene, view, call, renderer, &margins));
    if (view->nx * view->ny == 0u) return RTX_OK;
    Entry e(scene, device, Entry::kUploaded);
    if (e.rc != RTX_OK) return e.rc;
    DeviceState &st = e.state();
    RTX_TRY(frames_launch(scene, st, *view, call, renderer, margins.data(), sums, d_rgb, d_shade, nullptr, static_cast<hipStream_t>(stream)));
    return mark_uses(st, mean_uses(call), static_cast<hipStream_t>(stream));
}

// The bodies of rtx_render_view_rows and rtx_render_view_rows_device, each with its _lit twin's light as an argument (NULL:
// the scene's, nothing swapped) and its _posed twin's switch.  The host one renders into d_out on the library's stream and
// copies the rows back.  records (rtx_render_view_rows_shade): the output is RtxPixelShade records, 16 bytes a pixel in
// place of 3, through the record forms of the kernels that store a pixel; everything else is the byte call's.
int view_rows_host(RtxScene *scene, int device, const RtxView *view, const Lit *lit, bool posed, void *out, RtxStats *stats,
                   bool records = false)
{
    if (!view_rows_args_ok(scene, view, out)) return RTX_ERR_BAD_ARG;
    const Timed timed(stats);
    if (view->ny == 0u) return timed.empty();
    float shaft_delta = 0.0f;
    RTX_TRY(view_rows_supported(scene, view, lit, &shaft_delta));
    Entry e(scene, device, Entry::kUploaded);
    if (e.rc != RTX_OK) return e.rc;
    DeviceState &st = e.state();
    const RtxView v = *view;                 // (the caller's may change while the call runs)
    const size_t bytes = static_cast<size_t>(v.ny) * v.width * (records ? sizeof(RtxPixelShade) : 3u);
    RTX_TRY(st.d_out.reserve(bytes));
    DeviceGeometry *geo;
    RTX_TRY(geometry_of(st, posed, &geo));
    // a device-resident call may still read its light, make the pose, or walk what was aimed over it
    RTX_TRY(wait_for_uses(st, uses_of(lit, posed)));
    RTX_TRY(view_rows_launch(scene, st, *geo, v, st.d_out.as<uint8_t>(), timed.counters(st), st.stream, [&] { return timed.begin(st); },
                             lit, shaft_delta, records ? st.d_out.as<void>() : nullptr));
    RTX_TRY(timed.end(st));
    RTX_HIP(hipMemcpyAsync(out, st.d_out.as<void>(), bytes, hipMemcpyDeviceToHost, st.stream));
    return timed.gather(st, static_cast<uint64_t>(v.ny) * v.width * scene->prep.nb_ray, lit ? lit->count : scene->prep.nb_light_sample);
}

// ... the device-resident one into the caller's buffer on the caller's stream, nothing waited for
int view_rows_device(RtxScene *scene, int device, const RtxView *view, const Lit *lit, bool posed, void *d_rgb, size_t d_bytes,
                     void *stream, uint64_t *d_counters, bool records = false, const TileMask *mask = nullptr)
{
    if (!view_rows_args_ok(scene, view, d_rgb)) return RTX_ERR_BAD_ARG;
    if (records && reinterpret_cast<uintptr_t>(d_rgb) % sizeof(RtxPixelShade) != 0u) return RTX_ERR_BAD_ARG;
    if (d_bytes < static_cast<size_t>(view->ny) * view->width * (records ? sizeof(RtxPixelShade) : 3u)) return RTX_ERR_BAD_ARG;
    if (mask && (!records || !mask->d_tiles || (reinterpret_cast<uintptr_t>(mask->d_tiles) & 7u))) return RTX_ERR_BAD_ARG;
    if (view->ny == 0u) return RTX_OK;
    float shaft_delta = 0.0f;
    RTX_TRY(view_rows_supported(scene, view, lit, &shaft_delta));
    Entry e(scene, device, Entry::kUploaded);
    if (e.rc != RTX_OK) return e.rc;
    DeviceGeometry *geo;
    RTX_TRY(geometry_of(e.state(), posed, &geo));
    RTX_TRY(view_rows_launch(scene, e.state(), *geo, *view, static_cast<uint8_t *>(d_rgb), reinterpret_cast<unsigned long long *>(d_counters),
                             static_cast<hipStream_t>(stream), [] { return static_cast<int>(RTX_OK); }, lit, shaft_delta,
                             records ? d_rgb : nullptr, nullptr, 0u, mask));
    return mark_uses(e.state(), uses_of(lit, posed), static_cast<hipStream_t>(stream));
}

// Host statement of the pose kernels for what `c` states in host arrays (the overlay's with it): posed_records, or for a
// rebuilt pose rebuilt_records, which alone gives keys and perm.  The records are stated as the words the entry points give.
// Each output may be NULL.  May throw.
void records_on_host(const RtxScene *scene, const PoseCall &c, uint64_t *keys, uint32_t *perm, uint32_t *out_tris, uint32_t *out_shade,
                     uint32_t *out_nodes)
{
    RtxScene *sc = const_cast<RtxScene *>(scene);      // (the tables are caches under the scene's lock)
    const rtx::PoseTables &t = pose_tables_of(sc);
    rtx::TriRec *tris = reinterpret_cast<rtx::TriRec *>(out_tris);
    rtx::ShadeRec *shade = reinterpret_cast<rtx::ShadeRec *>(out_shade);
    rtx::NodeRec *nodes = reinterpret_cast<rtx::NodeRec *>(out_nodes);
    if (c.rebuilt) rtx::rebuilt_records(scene->prep, t, rebuild_tables_of(sc), c.v, c.tie_rank, keys, perm, tris, shade, nodes, &c.ov);
    else rtx::posed_records(scene->prep, t, c.v, c.tie_rank, tris, shade, nodes, &c.ov);
}

// host statement of the aim kernels over `nodes`, the scene's stream or a pose's, in place: stream_nearest_first from the
// tree proper's root; a scene without a primary stream of its own aims nothing, and the stream stays as it is
void nearest_first_on_host(const rtx::PreparedScene &p, std::vector<rtx::NodeRec> &nodes, const float eye[3])
{
    if (p.primary_nodes.empty()) return;
    std::vector<rtx::NodeRec> out;
    rtx::stream_nearest_first(nodes, tree_root(p, nodes.size()), eye, out);
    nodes.swap(out);
}

// host statement of the plane kernel and of the aim kernels over the pose `c` states: global_plane_statement over the posed
// records of the global triangles; nearest_first_on_host over the pose's node words, whose planes cull_delta has moved
// already (aimed: the uploaded stream's count of records, a rebuilt pose: the rebuilt stream's).  Each output may be NULL.
// May throw.
void posed_pipeline_on_host(const RtxScene *scene, const PoseCall &c, const float *eye, uint32_t *out_planes, uint32_t *aimed)
{
    const rtx::PreparedScene &p = scene->prep;
    std::vector<rtx::TriRec> tris(p.tris.size());
    std::vector<rtx::NodeRec> nodes(!aimed ? 0u : c.rebuilt ? rebuild_tables_of(const_cast<RtxScene *>(scene)).nodes.size() : p.nodes.size());
    records_on_host(scene, c, nullptr, nullptr, reinterpret_cast<uint32_t *>(tris.data()), nullptr,
                    aimed ? reinterpret_cast<uint32_t *>(nodes.data()) : nullptr);
    rtx::TriRec *planes = reinterpret_cast<rtx::TriRec *>(out_planes);
    if (planes)
        for (uint32_t i = 0; i < p.n_global; ++i) rtx::global_plane_statement(tris[i], planes + i);
    if (!aimed) return;
    nearest_first_on_host(p, nodes, eye);
    std::memcpy(aimed, nodes.data(), nodes.size() * sizeof(rtx::NodeRec));
}

// host statement of the aim kernels: the shadow stream with its planes moved as nodes_in_device_order moves them (f32),
// nearest first
std::vector<rtx::NodeRec> aimed_on_host(const rtx::PreparedScene &p, const float eye[3])
{
    std::vector<rtx::NodeRec> moved(p.nodes);
    const float inflate = p.cull_delta;
    for (rtx::NodeRec &n : moved)
        for (int k = 0; k < 3; ++k) {
            n.bmin[k] = n.bmin[k] - inflate;
            n.bmax[k] = n.bmax[k] + inflate;
        }
    nearest_first_on_host(p, moved, eye);
    return moved;
}

// The end of a read-back on the library's stream: n records of a node stream on the device (a geometry's nodes or its
// aimed stream) are copied behind what the call has enqueued, the stream is drained, and the records are stated in
// NodeRec word order, 8 words each.  out == NULL: no records, the stream is drained all the same.
int read_back_nodes(const DeviceState &st, const void *d_nodes, size_t n, uint32_t *out)
{
    std::vector<rtx::NodeDev> dev;
    try {
        dev.resize(out ? n : 0u);
    } catch (...) {
        (void)hipStreamSynchronize(st.stream);      // what the call has enqueued writes the caller's arrays
        return RTX_ERR_OOM;
    }
    if (!dev.empty()) RTX_HIP(hipMemcpyAsync(dev.data(), d_nodes, n * sizeof(rtx::NodeDev), hipMemcpyDeviceToHost, st.stream));
    RTX_HIP(hipStreamSynchronize(st.stream));
    for (size_t i = 0; i < dev.size(); ++i) {
        const rtx::NodeDev &d = dev[i];
        const rtx::NodeRec r{{d.lox, d.loy, d.loz}, d.link, {d.hix, d.hiy, d.hiz}, d.info};
        std::memcpy(out + 8u * i, &r, sizeof r);
    }
    return RTX_OK;
}

// ---- what a pose call is: one maker per family, each with all of that family's refusals in the order they apply --------
// host: the pointers are the host's, and reference_tree and the range rules apply; otherwise they are the device's, and the
// 4-byte alignment applies.  The flag word and the struct are looked at first, as every entry point did.

bool pose_head_ok(const RtxScene *scene, const void *in, uint32_t flags) { return scene && in && !(flags & ~RTX_POSE_REBUILT); }

// The refusals a maker ends with, over the arrays the call states itself: host form, pose_in_range and spheres_in_range;
// device form, every pointer of the call a multiple of 4.  (The device form looked at the moves' three pointers in a second
// condition with the same answer: one condition here, nothing to observe.)
int stated_arrays_ok(const RtxScene *scene, const PoseCall &c, bool host)
{
    if (host) {
        if (c.v && !rtx::pose_in_range(scene->prep, c.v)) return RTX_ERR_UNSUPPORTED;
        if (c.ov.spheres && !rtx::spheres_in_range(scene->prep, c.ov.spheres)) return RTX_ERR_UNSUPPORTED;
        return RTX_OK;
    }
    auto low_bits = [](auto... ptr) { return (reinterpret_cast<uintptr_t>(ptr) | ...); };
    return (low_bits(c.v, c.tie_rank, c.ov.spheres, c.ov.rgb, c.ov.sphere_rgb, c.moves.moves, c.moves.group, c.moves.radius_scale) & 3u)
               ? RTX_ERR_BAD_ARG : RTX_OK;
}

// rtx_scene_pose, rtx_scene_pose_rebuilt and their _device twins
int vertices_call(const RtxScene *scene, const void *v0v1v2, const void *tie_rank, bool rebuilt, bool host, uint32_t reference_tree,
                  PoseCall *call)
{
    if (!scene || !v0v1v2 || (host && reference_tree > RTX_REFTREE_NEVER)) return RTX_ERR_BAD_ARG;
    *call = vertices_alone(static_cast<const float *>(v0v1v2), static_cast<const uint32_t *>(tie_rank), rebuilt);
    return stated_arrays_ok(scene, *call, host);
}

// What rtx_scene_pose_prims reads of its struct for `scene`: the arrays of an arm the scene does not have are not read.
// RTX_ERR_BAD_ARG for vertices missing with triangles present.
int prims_of(const RtxScene *scene, const RtxPosePrims *in, uint32_t flags, PoseCall *call)
{
    const bool triangles = posed_triangles(scene) != 0u, spheres = scene->prep.n_spheres != 0u;
    if (triangles && !in->v0v1v2) return RTX_ERR_BAD_ARG;
    call->v = triangles ? in->v0v1v2 : nullptr;
    call->tie_rank = in->tie_rank;
    call->ov.rgb = triangles ? in->rgb : nullptr;
    call->ov.spheres = spheres ? in->spheres : nullptr;
    call->ov.sphere_rgb = spheres ? in->sphere_rgb : nullptr;
    call->spheres = call->ov.spheres != nullptr;
    call->rebuilt = (flags & RTX_POSE_REBUILT) != 0u;
    return RTX_OK;
}

// rtx_scene_pose_prims and its _device twin
int prims_call(const RtxScene *scene, const RtxPosePrims *in, uint32_t flags, bool host, uint32_t reference_tree, PoseCall *call)
{
    if (!pose_head_ok(scene, in, flags)) return RTX_ERR_BAD_ARG;
    RTX_TRY(prims_of(scene, in, flags, call));
    if (host && reference_tree > RTX_REFTREE_NEVER) return RTX_ERR_BAD_ARG;
    return stated_arrays_ok(scene, *call, host);
}

// What rtx_scene_pose_moved reads of its struct for `scene`, as prims_of: the colours of an arm the scene does not have are
// not read, and the pose states spheres where the scene has some.  RTX_ERR_BAD_ARG for a NULL `moves` or a count outside
// 1 ... 65,536.
int moves_of(const RtxScene *scene, const RtxPoseMoves *in, uint32_t flags, PoseCall *call)
{
    if (!in->moves || in->n_moves == 0u || in->n_moves > rtx::kMaxMoves) return RTX_ERR_BAD_ARG;
    call->moves.n_moves = in->n_moves;
    call->moves.moves = in->moves;
    call->moves.group = in->group;
    call->moves.radius_scale = in->radius_scale;
    call->tie_rank = in->tie_rank;
    call->ov.rgb = posed_triangles(scene) != 0u ? in->rgb : nullptr;
    call->ov.sphere_rgb = scene->prep.n_spheres != 0u ? in->sphere_rgb : nullptr;
    call->spheres = scene->prep.n_spheres != 0u;
    call->rebuilt = (flags & RTX_POSE_REBUILT) != 0u;
    return RTX_OK;
}

// rtx_scene_pose_moved and its _device twin.  The host form applies the range rule to the statement (rtx::moved_in_range),
// nothing stored.  rtx_scene_moved_prims does not look at the groups; neither does the device form.
int moved_call(const RtxScene *scene, const RtxPoseMoves *in, uint32_t flags, bool host, uint32_t reference_tree, PoseCall *call)
{
    if (!pose_head_ok(scene, in, flags) || (host && reference_tree > RTX_REFTREE_NEVER)) return RTX_ERR_BAD_ARG;
    RTX_TRY(moves_of(scene, in, flags, call));
    if (!host) return stated_arrays_ok(scene, *call, false);
    if (!rtx::move_groups_ok(scene->prep, call->moves)) return RTX_ERR_BAD_ARG;
    return rtx::moved_in_range(scene->prep, call->moves) ? RTX_OK : RTX_ERR_UNSUPPORTED;
}

// rtx_scene_pose_skinned and its _device twin: the moves are blended per corner by the scene's skin.  n_moves against the
// bind's largest bone is O(1), what the bind recorded, and the host form's alone: the kernel takes a bone at or above the
// count as RTX_MOVE_NONE.
int skinned_call(const RtxScene *scene, const RtxPoseMoves *in, uint32_t flags, bool host, uint32_t reference_tree, PoseCall *call)
{
    if (!pose_head_ok(scene, in, flags) || (host && reference_tree > RTX_REFTREE_NEVER)) return RTX_ERR_BAD_ARG;
    RTX_TRY(moves_of(scene, in, flags, call));
    const rtx::Skin &skin = scene->skin;
    if (call->moves.group || !skin.bound || (host && call->moves.n_moves <= skin.max_bone)) return RTX_ERR_BAD_ARG;
    call->skin = &skin;
    if (!host) return stated_arrays_ok(scene, *call, false);
    return rtx::skinned_in_range(scene->prep, skin, call->moves) ? RTX_OK : RTX_ERR_UNSUPPORTED;
}

// The body of the five host entry points, `c` made by its family's maker: the reference's own tree where reference_tree asks
// for one — over the call's arrays, a moved pose's made by the host statement for this alone —, the reservations, the
// copies onto the library's stream, and pose_launch over the copies.
int pose_host(RtxScene *scene, int device, const PoseCall &c, uint32_t reference_tree, RtxStats *stats)
{
    const rtx::PreparedScene &p = scene->prep;
    const Timed timed(stats);
    Entry e(scene, device, Entry::kUploaded);
    if (e.rc != RTX_OK) return e.rc;
    DeviceState &st = e.state();
    const size_t n_prims = p.tris.size(), n_triangles = posed_triangles(scene);
    const bool want_ref = reference_tree == RTX_REFTREE_ALWAYS || (reference_tree == RTX_REFTREE_AUTO && n_prims <= rtx::kRefTreeAutoMax);
    std::vector<uint32_t> ref_rank;
    std::vector<rtx::NodeDev> ref_stream;
    try {
        if (want_ref) {
            std::vector<float> moved_v(c.moved() ? p.rest_v0v1v2.size() : 0u), moved_spheres(c.moved() ? p.rest_spheres.size() : 0u);
            PoseCall stated = c;      // the call in host arrays
            if (c.skin) rtx::skinned_prims(p, *c.skin, c.moves, moved_v.data(), moved_spheres.data());
            else if (c.moved()) rtx::moved_prims(p, c.moves, moved_v.data(), moved_spheres.data());
            if (c.moved()) {
                stated.v = moved_v.data();
                if (p.n_spheres) stated.ov.spheres = moved_spheres.data();
            }
            const rtx::PrimsOverlay *ov = c.overlaid() ? &stated.ov : nullptr;
            std::vector<rtx::NodeRec> stream;
            if (c.rebuilt) {      // the leaves name positions of the sorted array: through the host statement's permutation
                std::vector<uint32_t> perm(n_prims - p.n_global);
                rtx::rebuilt_records(p, pose_tables_of(scene), rebuild_tables_of(scene), stated.v, nullptr, nullptr, perm.data(), nullptr,
                                     nullptr, nullptr, ov);
                RTX_TRY(rtx::rebuilt_ref_tree(p, pose_tables_of(scene), stated.v, perm.data(), ref_rank, stream, ov));
            } else {
                RTX_TRY(rtx::posed_ref_tree(p, pose_tables_of(scene), stated.v, ref_rank, stream, ov));
            }
            ref_stream = rtx::nodes_in_device_order(stream);
        }
    } catch (...) {
        return RTX_ERR_OOM;
    }
    const uint32_t *rank = c.tie_rank ? c.tie_rank : (want_ref ? ref_rank.data() : nullptr);
    RTX_TRY(reserve_pose(scene, st, true, ref_stream.size(), c.rebuilt));
    if (c.overlaid()) RTX_TRY(reserve_prims(scene, st, true, c));
    if (c.moved()) RTX_TRY(reserve_moves(scene, st, true, c.moves));
    if (c.skin) RTX_TRY(reserve_skin(scene, st));
    RTX_TRY(wait_for_uses(st, kUsesPose));      // a device-resident call may still read the pose this one replaces
    if (!c.moved()) st.pose.f.ran = false;      // (the copies below overwrite what the move kernel wrote)
    hipError_t he = hipSuccess;
    auto copy_in = [&](const auto *from, DeviceBuffer &to, size_t n) {      // -> the copy (an array not given: nothing, NULL)
        using T = std::remove_cv_t<std::remove_pointer_t<decltype(from)>>;
        if (!from) return static_cast<const T *>(nullptr);
        if (he == hipSuccess && n) he = hipMemcpyAsync(to.as<void>(), from, n * sizeof(T), hipMemcpyHostToDevice, st.stream);
        return to.as<const T>();
    };
    PoseCall d = c;      // the call over the library's copies
    copy_in(c.v, st.pose.v, n_triangles * 9u);
    d.v = st.pose.v.as<const float>();
    d.moves.moves = copy_in(c.moves.moves, st.pose.f.moves, static_cast<size_t>(c.moves.n_moves) * 12u);
    d.moves.group = copy_in(c.moves.group, st.pose.f.group, n_prims);
    d.moves.radius_scale = copy_in(c.moves.radius_scale, st.pose.f.radius_scale, c.moves.n_moves);
    d.ov.spheres = copy_in(c.ov.spheres, st.pose.m.spheres, static_cast<size_t>(p.n_spheres) * 4u);
    d.ov.rgb = copy_in(c.ov.rgb, st.pose.m.rgb, n_triangles * 3u);
    d.ov.sphere_rgb = copy_in(c.ov.sphere_rgb, st.pose.m.sphere_rgb, static_cast<size_t>(p.n_spheres) * 3u);
    d.tie_rank = copy_in(rank, st.pose.rank, n_prims);
    if (he == hipSuccess && !ref_stream.empty()) {
        he = hipMemcpyAsync(st.pose.geo.ref_nodes.as<void>(), ref_stream.data(), ref_stream.size() * sizeof(rtx::NodeDev),
                            hipMemcpyHostToDevice, st.stream);
        if (he == hipSuccess)
            he = hipMemsetAsync(st.pose.geo.ref_nodes.as<rtx::NodeDev>() + ref_stream.size(), 0, sizeof(rtx::NodeDev), st.stream);
    }
    int rc = hip_rc(he);
    if (rc == RTX_OK) rc = timed.begin(st);
    if (rc == RTX_OK) rc = pose_launch(scene, st, d, st.stream);
    if (rc == RTX_OK) rc = timed.end(st);
    if (rc != RTX_OK) {
        st.pose.valid = false;
        (void)hipStreamSynchronize(st.stream);      // the copies above read the caller's arrays and this call's vectors
        return rc;
    }
    st.pose.geo.n_ref_nodes = static_cast<uint32_t>(ref_stream.size());
    return timed.gather(st, 0u, 0u);
}

// ... of the five device-resident ones: the reservations and pose_launch over the caller's arrays on the caller's stream,
// nothing waited for.  (The overlay's primitive records are reserved where spheres are stated, the move kernel's too.)
int pose_device(RtxScene *scene, int device, const PoseCall &d, void *stream)
{
    Entry e(scene, device, Entry::kUploaded);
    if (e.rc != RTX_OK) return e.rc;
    DeviceState &st = e.state();
    RTX_TRY(reserve_pose(scene, st, false, 0u, d.rebuilt));
    if (d.moved()) RTX_TRY(reserve_moves(scene, st, false, d.moves));
    if (d.skin) RTX_TRY(reserve_skin(scene, st));
    if (d.overlaid()) RTX_TRY(reserve_prims(scene, st, false, d));
    RTX_TRY(pose_launch(scene, st, d, static_cast<hipStream_t>(stream)));
    return mark_uses(st, kUsesPose, static_cast<hipStream_t>(stream));
}

// The end of a pose's read-back with an aimed stream: the aim kernels run over `g` for `eye`, whatever the buffer holds, and
// the n records of their stream are read back (read_back_nodes; out == NULL: nothing is aimed, the stream is drained)
int read_back_aimed(RtxScene *scene, DeviceState &st, DeviceGeometry &g, const float eye[3], size_t n, uint32_t *out)
{
    if (out && n) {
        RTX_TRY(reserve_aimed(scene, g));
        g.aimed.valid = false;
        RTX_TRY(aim_at(scene, g, eye, st.stream));
    }
    return read_back_nodes(st, aimed_stream(scene, g), n, out);
}

// a host statement, which may throw std::bad_alloc, as a return code
template <class Statement>
int on_host(Statement statement)
{
    try {
        statement();
    } catch (...) {
        return RTX_ERR_OOM;
    }
    return RTX_OK;
}

// The body of rtx_debug_pose and of rtx_debug_pose_rebuilt (for_rebuilt), each with its own refusal: the first states its
// nodes by the uploaded count and so gives none of a rebuilt pose, the second reads a rebuilt pose alone.  The records of
// the pose the device holds are copied back behind what a device-resident pose has enqueued; the second then runs the aim
// kernels over the pose for `eye` and reads their stream.  Each output may be NULL.
int debug_pose(RtxScene *scene, int device, bool for_rebuilt, const float *eye, uint32_t *out_perm, uint32_t *out_tris,
               uint32_t *out_shade, uint32_t *out_nodes, uint32_t *out_aimed)
{
    if (!scene || (out_aimed && !eye)) return RTX_ERR_BAD_ARG;
    Entry e(scene, device, Entry::kUploaded);
    if (e.rc != RTX_OK) return e.rc;
    DeviceState &st = e.state();
    DeviceGeometry *g;
    RTX_TRY(geometry_of(st, true, &g));
    if (for_rebuilt ? !st.pose.rebuilt : (st.pose.rebuilt && out_nodes)) return RTX_ERR_BAD_ARG;
    const size_t n_prims = scene->prep.tris.size(), n_tree = n_prims - scene->prep.n_global, n = g->n_nodes;
    RTX_TRY(wait_for_uses(st, kUsesPose));
    if (out_perm && n_tree)
        RTX_HIP(hipMemcpyAsync(out_perm, st.pose.b.perm.as<void>(), n_tree * sizeof(uint32_t), hipMemcpyDeviceToHost, st.stream));
    if (out_tris) RTX_HIP(hipMemcpyAsync(out_tris, g->tris.as<void>(), n_prims * sizeof(rtx::TriRec), hipMemcpyDeviceToHost, st.stream));
    if (out_shade)
        RTX_HIP(hipMemcpyAsync(out_shade, g->shade.as<void>(), n_prims * sizeof(rtx::ShadeRec), hipMemcpyDeviceToHost, st.stream));
    if (!for_rebuilt) return read_back_nodes(st, g->nodes.as<void>(), n, out_nodes);      // (refitted: n is the uploaded count)
    RTX_TRY(read_back_nodes(st, g->nodes.as<void>(), n, out_nodes));
    return read_back_aimed(scene, st, *g, eye, n, out_aimed);
}

}  // namespace

extern "C" {

int rtx_abi_version(void) { return RTX_ABI_VERSION; }

int rtx_device_count(void) { return device_count_quiet(); }

int rtx_last_hip_error(void) { return g_last_hip_error; }

const char *rtx_strerror(int err)
{
    switch (err) {
    case RTX_OK: return "ok";
    case RTX_ERR_BAD_ARG: return "bad argument";
    case RTX_ERR_NO_DEVICE: return "no usable HIP device (there is no CPU fallback)";
    case RTX_ERR_HIP: return "HIP runtime error";
    case RTX_ERR_OOM: return "out of memory";
    case RTX_ERR_UNSUPPORTED: return "unsupported input";
    case RTX_ERR_INTERNAL: return "internal error";
    case RTX_ERR_IO: return "I/O or parse error";
    default: return "unknown error";
    }
}

int rtx_scene_create(const RtxSceneDesc *desc, RtxScene **out)
{
    if (!desc || !out) return RTX_ERR_BAD_ARG;
    *out = nullptr;
    RtxScene *s = new (std::nothrow) RtxScene;
    if (!s) return RTX_ERR_OOM;
    int rc;
    try {
        rc = rtx::prepare_scene(*desc, s->prep);
    } catch (...) {
        rc = RTX_ERR_INTERNAL;
    }
    if (rc != RTX_OK) { delete s; return rc; }
    *out = s;
    return RTX_OK;
}

void rtx_scene_destroy(RtxScene *scene)
{
    delete scene;      // every device's state goes through ReleaseOnDevice, in ascending device id
}

int rtx_scene_info(const RtxScene *scene, RtxSceneInfo *info)
{
    if (!scene || !info) return RTX_ERR_BAD_ARG;
    const rtx::PreparedScene &p = scene->prep;
    info->n_tris = p.n_tris;
    info->n_nodes = static_cast<uint32_t>(p.nodes.size());
    info->n_leaves = p.n_leaves;
    info->max_leaf_tris = p.max_leaf_tris;
    info->depth = p.depth;
    info->n_light_points = p.nb_ray * p.nb_light_sample;
    info->n_ref_nodes = static_cast<uint32_t>(p.ref_nodes.size());
    info->n_global = p.n_global;
    info->node_bytes = p.nodes.size() * sizeof(rtx::NodeRec);
    info->tri_bytes = p.tris.size() * sizeof(rtx::TriRec);
    info->shade_bytes = p.shade.size() * sizeof(rtx::ShadeRec);
    info->sample_bytes = 2u * static_cast<uint64_t>(p.n_samples) * sizeof(float);
    return RTX_OK;
}

int rtx_scene_upload(RtxScene *scene, int device)
{
    if (!scene) return RTX_ERR_BAD_ARG;
    return Entry(scene, device, Entry::kUploaded).rc;
}

int rtx_render_rows(RtxScene *scene, int device, uint32_t row0, uint32_t nrows, uint8_t *out_rgb, RtxStats *stats)
{
    if (!scene || !out_rgb) return RTX_ERR_BAD_ARG;
    const uint32_t H = scene->prep.height, W = scene->prep.width;
    if (row0 > H || nrows > H - row0) return RTX_ERR_BAD_ARG;
    const Timed timed(stats);
    Entry e(scene, device, Entry::kCurrent);
    if (e.rc != RTX_OK) return e.rc;
    if (nrows == 0) return timed.empty();
    RTX_TRY(launch_on(scene, *e.slot, rtx::TileSpec{row0, nrows, nrows, nrows}, timed));
    const DeviceState &st = e.state();
    const uint64_t pixels = static_cast<uint64_t>(nrows) * W;
    RTX_HIP(hipMemcpyAsync(out_rgb, st.d_out.as<void>(), pixels * 3u, hipMemcpyDeviceToHost, st.stream));
    return timed.gather(st, pixels * scene->prep.nb_ray, scene->prep.nb_light_sample);
}

int rtx_render_frame(RtxScene *scene, const int *devices, int n_devices, uint32_t tile_rows,
                     uint8_t *out_rgb, RtxStats *stats)
{
    if (!scene || !devices || n_devices <= 0 || !tile_rows || !out_rgb) return RTX_ERR_BAD_ARG;
    // first_row / stride of a share are 32-bit row numbers (rtx_render_tiles_device checks the same)
    if (static_cast<uint64_t>(n_devices) * tile_rows > 0xFFFFFFFFull) return RTX_ERR_BAD_ARG;
    const uint32_t H = scene->prep.height, W = scene->prep.width;
    const size_t row_bytes = static_cast<size_t>(W) * 3u;
    const double t0 = wall_ms();
    // Share j = row tiles j, j + n, ... goes to devices[j].  A device may be named more than once: its shares are
    // then rendered one after another on its stream (this is also how the path is rehearsed on a one-GPU box).
    struct Share { DeviceSlot *slot; rtx::TileSpec spec; size_t stage_offset; };
    std::vector<Share> shares(static_cast<size_t>(n_devices));
    std::map<int, DeviceSlot *> unique;                    // ascending device id: the order the locks are taken in, so
    for (int j = 0; j < n_devices; ++j) {                  // that concurrent calls naming {0,1} and {1,0} cannot deadlock
        const int rc = get_slot(scene, devices[j], &shares[j].slot);
        if (rc != RTX_OK) return rc;
        unique[devices[j]] = shares[j].slot;
    }
    std::vector<std::unique_lock<std::mutex>> locks;
    for (auto &kv : unique) locks.emplace_back(kv.second->mu);
    // per device: the largest share (device buffer) and the sum of its shares (pinned staging), sized BEFORE anything is
    // in flight — growing a buffer later would free memory a copy is still reading
    std::map<DeviceSlot *, std::pair<size_t, size_t>> need;
    for (int j = 0; j < n_devices; ++j) {
        const uint32_t rows = tiles_rows(H, static_cast<uint32_t>(j), static_cast<uint32_t>(n_devices), tile_rows);
        shares[j].spec = rtx::TileSpec{static_cast<uint32_t>(j) * tile_rows, tile_rows,
                                       static_cast<uint32_t>(n_devices) * tile_rows, rows};
        auto &n = need[shares[j].slot];
        shares[j].stage_offset = n.second;
        n.first = std::max(n.first, rows * row_bytes);
        n.second += rows * row_bytes;
    }
    // on any failure: wait for what was already launched (kernels and copies into our staging buffers) before returning
    std::vector<int> launched;
    auto fail = [&](int rc) {
        for (int d : launched) {
            DeviceGuard g(d);
            if (g.status() == hipSuccess) (void)hipStreamSynchronize(unique[d]->st->stream);
        }
        return rc;
    };
    for (auto &kv : unique) {
        DeviceGuard g(kv.first);
        RTX_HIP(g.status());
        const auto &n = need[kv.second];
        int rc = ensure_state(*kv.second, kv.first);
        if (rc != RTX_OK) return rc;
        // uploaded, and caught up with a replaced sample table, before any share is launched anywhere
        if ((rc = ensure_uploaded(scene, *kv.second)) != RTX_OK) return rc;
        if ((rc = kv.second->st->d_out.reserve(n.first ? n.first : 16)) != RTX_OK) return rc;
        if ((rc = kv.second->st->h_stage.reserve(n.second ? n.second : 16)) != RTX_OK) return rc;
    }
    // launch everywhere first (asynchronous), then gather
    unsigned long long total[rtx::kNumCounters] = {0};
    std::vector<unsigned long long> counters(static_cast<size_t>(n_devices) * rtx::kNumCounters, 0ull);
    std::vector<float> share_ms(static_cast<size_t>(n_devices), 0.0f);
    for (int j = 0; j < n_devices; ++j) {
        Share &sh = shares[j];
        if (!sh.spec.local_rows) continue;
        DeviceGuard g(devices[j]);
        if (g.status() != hipSuccess) return fail(hip_rc(g.status()));
        const int rc = launch_on(scene, *sh.slot, sh.spec, Timed(stats));      // (the frame gathers and times its shares itself)
        if (rc != RTX_OK) return fail(rc);
        launched.push_back(devices[j]);
        DeviceState &st = *sh.slot->st;
        hipError_t e = hipMemcpyAsync(st.h_stage.as<uint8_t>() + sh.stage_offset, st.d_out.as<void>(), sh.spec.local_rows * row_bytes,
                                      hipMemcpyDeviceToHost, st.stream);
        if (e == hipSuccess && stats)   // a device's next share reuses its counter block: read this share's now (stream order)
            e = hipMemcpyAsync(&counters[static_cast<size_t>(j) * rtx::kNumCounters], st.d_counters.as<void>(),
                               rtx::kNumCounters * sizeof(unsigned long long), hipMemcpyDeviceToHost, st.stream);
        if (e != hipSuccess) return fail(hip_rc(e));
        if (stats && unique.size() != static_cast<size_t>(n_devices)) {
            // shares of one device run back to back and share its two timing events: take each share's time now
            if ((e = hipStreamSynchronize(st.stream)) != hipSuccess || (e = hipEventElapsedTime(&share_ms[j], st.ev0, st.ev1)) != hipSuccess)
                return fail(hip_rc(e));
        }
    }
    double kernel_ms = 0.0;
    for (auto &kv : unique) {
        DeviceGuard g(kv.first);
        if (g.status() != hipSuccess) return fail(hip_rc(g.status()));
        const hipError_t e = hipStreamSynchronize(kv.second->st->stream);
        if (e != hipSuccess) return fail(hip_rc(e));
    }
    for (int j = 0; j < n_devices; ++j) {
        const Share &sh = shares[j];
        if (!sh.spec.local_rows) continue;
        // the packed tiles of this share go to their rows of the frame (disjoint rows per share)
        rtxh_scatter_tiles(out_rgb, H, W, sh.slot->st->h_stage.as<uint8_t>() + sh.stage_offset, static_cast<uint32_t>(j), static_cast<uint32_t>(n_devices), tile_rows);
        if (stats) {
            if (unique.size() == static_cast<size_t>(n_devices)) {
                DeviceGuard g(devices[j]);
                float ms = 0.0f;
                if (g.status() == hipSuccess && hipEventElapsedTime(&ms, sh.slot->st->ev0, sh.slot->st->ev1) == hipSuccess) share_ms[j] = ms;
            }
            for (int k = 0; k < rtx::kNumCounters; ++k) total[k] += counters[static_cast<size_t>(j) * rtx::kNumCounters + k];
        }
    }
    if (stats) {
        // the frame's device time: the slowest device, a device's shares added up
        std::map<DeviceSlot *, double> per_device;
        for (int j = 0; j < n_devices; ++j) per_device[shares[j].slot] += share_ms[j];
        for (auto &kv : per_device) kernel_ms = std::max(kernel_ms, kv.second);
        fill_stats(stats, static_cast<uint64_t>(H) * W * scene->prep.nb_ray, scene->prep.nb_light_sample, total, kernel_ms, wall_ms() - t0);
    }
    return RTX_OK;
}

uint32_t rtx_tiles_rows(const RtxScene *scene, uint32_t first_tile, uint32_t tile_stride, uint32_t tile_rows)
{
    return scene ? tiles_rows(scene->prep.height, first_tile, tile_stride, tile_rows) : 0;
}

size_t rtx_tiles_bytes(const RtxScene *scene, uint32_t first_tile, uint32_t tile_stride, uint32_t tile_rows)
{
    return scene ? static_cast<size_t>(tiles_rows(scene->prep.height, first_tile, tile_stride, tile_rows)) *
                       scene->prep.width * 3u
                 : 0;
}

int rtx_render_tiles_device(RtxScene *scene, int device, uint32_t first_tile, uint32_t tile_stride,
                            uint32_t tile_rows, void *d_out_rgb, size_t d_out_bytes, void *stream,
                            uint64_t *d_counters)
{
    if (!scene || !d_out_rgb || !tile_rows || !tile_stride) return RTX_ERR_BAD_ARG;
    const uint32_t rows = tiles_rows(scene->prep.height, first_tile, tile_stride, tile_rows);
    if (static_cast<size_t>(rows) * scene->prep.width * 3u > d_out_bytes) return RTX_ERR_BAD_ARG;
    if (static_cast<uint64_t>(first_tile) * tile_rows > 0xFFFFFFFFull ||
        static_cast<uint64_t>(tile_stride) * tile_rows > 0xFFFFFFFFull) return RTX_ERR_BAD_ARG;
    Entry e(scene, device, Entry::kUploaded);
    if (e.rc != RTX_OK) return e.rc;
    const rtx::TileSpec ts{first_tile * tile_rows, tile_rows, tile_stride * tile_rows, rows};
    const rtx::DeviceScene S = device_scene(scene, e.state(), e.state().geo);
    rtx::ProbeSplit split;
    RTX_TRY(probe_split_of(scene, e.state(), S, ts, &split));
    return render_launch(e.state(), S, ts, static_cast<uint8_t *>(d_out_rgb),
                         reinterpret_cast<unsigned long long *>(d_counters), nullptr, static_cast<hipStream_t>(stream),
                         [] { return static_cast<int>(RTX_OK); }, split);
}

int rtx_trace_rays(RtxScene *scene, int device, uint32_t n_rays, const float *origins, const float *directions,
                   uint32_t flags, RtxRayHit *out_hits, RtxStats *stats)
{
    if (!query_args_ok(scene, origins, directions, out_hits, flags, n_rays)) return RTX_ERR_BAD_ARG;
    return batch_host(scene, device, query_batch(false, n_rays, flags, false), origins, directions, {out_hits, nullptr, nullptr}, stats);
}

int rtx_occluded_rays(RtxScene *scene, int device, uint32_t n_rays, const float *origins, const float *targets,
                      uint32_t flags, uint8_t *out_occluded, RtxStats *stats)
{
    if (!query_args_ok(scene, origins, targets, out_occluded, flags, n_rays)) return RTX_ERR_BAD_ARG;
    return batch_host(scene, device, query_batch(true, n_rays, flags, false), origins, targets, {out_occluded, nullptr, nullptr}, stats);
}

int rtx_trace_rays_device(RtxScene *scene, int device, uint32_t n_rays, const void *d_origins, const void *d_directions,
                          uint32_t flags, void *d_hits, void *stream)
{
    if (!query_args_ok(scene, d_origins, d_directions, d_hits, flags, n_rays) || !aligned16(d_hits)) return RTX_ERR_BAD_ARG;
    return batch_device(scene, device, query_batch(false, n_rays, flags, false), d_origins, d_directions, {d_hits, nullptr, nullptr}, stream);
}

int rtx_occluded_rays_device(RtxScene *scene, int device, uint32_t n_rays, const void *d_origins, const void *d_targets,
                             uint32_t flags, void *d_occluded, void *stream)
{
    if (!query_args_ok(scene, d_origins, d_targets, d_occluded, flags, n_rays)) return RTX_ERR_BAD_ARG;
    return batch_device(scene, device, query_batch(true, n_rays, flags, false), d_origins, d_targets, {d_occluded, nullptr, nullptr}, stream);
}

int rtx_shade_rays(RtxScene *scene, int device, uint32_t n_pixels, const float *origins, const float *directions,
                   uint32_t flags, RtxPixelShade *out_shade, RtxRayHit *out_hits, RtxStats *stats)
{
    return shade_host(scene, device, n_pixels, origins, directions, flags, nullptr, false, out_shade, out_hits, stats);
}

int rtx_shade_rays_device(RtxScene *scene, int device, uint32_t n_pixels, const void *d_origins, const void *d_directions,
                          uint32_t flags, void *d_shade, void *d_hits, void *stream)
{
    return shade_device(scene, device, n_pixels, d_origins, d_directions, flags, nullptr, false, d_shade, d_hits, stream);
}

int rtx_scene_view(const RtxScene *scene, RtxView *out)
{
    if (!scene || !out) return RTX_ERR_BAD_ARG;
    const rtx::PreparedScene &p = scene->prep;
    std::memset(out, 0, sizeof *out);
    out->width = out->nx = p.width;
    out->height = out->ny = p.height;
    std::memcpy(out->eye, p.eye, 12);
    std::memcpy(out->u, p.cam_u, 12);
    std::memcpy(out->v, p.cam_v, 12);
    std::memcpy(out->w, p.cam_w, 12);
    out->distance = p.distance;
    return RTX_OK;
}

int rtx_render_view(RtxScene *scene, int device, const RtxView *view, uint8_t *out_rgb, RtxPixelShade *out_shade,
                    RtxRayHit *out_hits, RtxStats *stats)
{
    return view_host(scene, device, view, nullptr, false, out_rgb, out_shade, out_hits, stats);
}

int rtx_render_view_device(RtxScene *scene, int device, const RtxView *view, void *d_rgb, void *d_shade, void *d_hits,
                           void *stream)
{
    return view_device(scene, device, view, nullptr, false, d_rgb, d_shade, d_hits, stream);
}

int rtx_scene_light(const RtxScene *scene, RtxLight *out)
{
    if (!scene || !out) return RTX_ERR_BAD_ARG;
    const rtx::PreparedScene &p = scene->prep;
    std::memcpy(out->v0, p.light_v, 12);
    std::memcpy(out->v1, p.light_v + 3, 12);
    std::memcpy(out->v2, p.light_v + 6, 12);
    out->nb_light_sample = p.nb_light_sample;
    return RTX_OK;
}

int rtx_render_view_lit(RtxScene *scene, int device, const RtxView *view, const RtxLight *light, uint8_t *out_rgb,
                        RtxPixelShade *out_shade, RtxRayHit *out_hits, RtxStats *stats)
{
    const CallLight l(scene, light, CallLight::kRequired);
    return l.ok ? view_host(scene, device, view, l.lit, false, out_rgb, out_shade, out_hits, stats) : RTX_ERR_BAD_ARG;
}

int rtx_render_view_lit_device(RtxScene *scene, int device, const RtxView *view, const RtxLight *light, void *d_rgb,
                               void *d_shade, void *d_hits, void *stream)
{
    const CallLight l(scene, light, CallLight::kRequired);
    return l.ok ? view_device(scene, device, view, l.lit, false, d_rgb, d_shade, d_hits, stream) : RTX_ERR_BAD_ARG;
}

int rtx_shade_rays_lit(RtxScene *scene, int device, uint32_t n_pixels, const float *origins, const float *directions,
                       uint32_t flags, const RtxLight *light, RtxPixelShade *out_shade, RtxRayHit *out_hits, RtxStats *stats)
{
    const CallLight l(scene, light, CallLight::kRequired);
    return l.ok ? shade_host(scene, device, n_pixels, origins, directions, flags, l.lit, false, out_shade, out_hits, stats) : RTX_ERR_BAD_ARG;
}

int rtx_shade_rays_lit_device(RtxScene *scene, int device, uint32_t n_pixels, const void *d_origins, const void *d_directions,
                              uint32_t flags, const RtxLight *light, void *d_shade, void *d_hits, void *stream)
{
    const CallLight l(scene, light, CallLight::kRequired);
    return l.ok ? shade_device(scene, device, n_pixels, d_origins, d_directions, flags, l.lit, false, d_shade, d_hits, stream) : RTX_ERR_BAD_ARG;
}

int rtx_scene_light_points_for(const RtxScene *scene, const RtxLight *light, float *out)
{
    Lit lit;
    if (!lit_of(scene, light, &lit)) return RTX_ERR_BAD_ARG;
    const rtx::PreparedScene &p = scene->prep;
    if (out) rtx::light_points_of(lit.tri.v, rtx::sample_source(p), p.nb_ray, lit.count, out);
    return static_cast<int>(p.nb_ray * lit.count);      // <= 2^20
}

int rtx_debug_light_points(RtxScene *scene, int device, const RtxLight *light, float *out)
{
    Lit lit;
    if (!out || !lit_of(scene, light, &lit)) return RTX_ERR_BAD_ARG;
    if (!light_is_finite(lit)) return RTX_ERR_UNSUPPORTED;
    Entry e(scene, device, Entry::kUploaded);
    if (e.rc != RTX_OK) return e.rc;
    DeviceState &st = e.state();
    RTX_TRY(reserve_light(scene, st, lit, false));
    RTX_TRY(wait_for_uses(st, kUsesLight));
    RTX_TRY(light_launch(scene, st, lit, false, st.stream));
    const size_t bytes = static_cast<size_t>(scene->prep.nb_ray) * lit.count * 3u * sizeof(float);
    if (bytes) RTX_HIP(hipMemcpyAsync(out, st.lit.points.as<void>(), bytes, hipMemcpyDeviceToHost, st.stream));
    RTX_HIP(hipStreamSynchronize(st.stream));
    return RTX_OK;
}

// ---- the sample table replaced (rtx_scene_resample, rtx_scene_reseed; the kernel: rtx_samples.hip) -------------------------
// Host only, and like rtx_scene_skin not re-entrant per handle: the scene is read and written without a lock.  Each device
// catches up in its next call (ensure_uploaded).

int rtx_scene_resample(RtxScene *scene, const float *samples, uint32_t n_samples)
{
    if (!scene || !samples || !n_samples) return RTX_ERR_BAD_ARG;
    return rtx::resample_scene(scene->prep, rtx::SampleSource{samples, 0u, n_samples});
}

int rtx_scene_reseed(RtxScene *scene, uint64_t seed, uint32_t n_pairs)
{
    if (!scene || !n_pairs) return RTX_ERR_BAD_ARG;
    return rtx::resample_scene(scene->prep, rtx::SampleSource{nullptr, seed, n_pairs});
}

// first + count within the table, or RTX_ERR_BAD_ARG
static int sample_range_ok(const RtxScene *scene, uint64_t first, uint32_t count, const float *out)
{
    if (!scene || (count && !out)) return RTX_ERR_BAD_ARG;
    const uint64_t n = scene->prep.n_samples;
    return first <= n && count <= n - first ? RTX_OK : RTX_ERR_BAD_ARG;
}

int rtx_scene_samples(const RtxScene *scene, uint64_t first, uint32_t count, float *out)
{
    RTX_TRY(sample_range_ok(scene, first, count, out));
    const rtx::SampleSource src = rtx::sample_source(scene->prep);
    for (uint64_t k = 0; k < count; ++k) src.pair(first + k, &out[2 * k], &out[2 * k + 1]);
    return RTX_OK;
}

int rtx_debug_samples(RtxScene *scene, int device, uint64_t first, uint32_t count, float *out)
{
    RTX_TRY(sample_range_ok(scene, first, count, out));
    Entry e(scene, device, Entry::kUploaded);
    if (e.rc != RTX_OK) return e.rc;
    const DeviceState &st = e.state();
    RTX_HIP(hipStreamSynchronize(st.stream));
    if (count) RTX_HIP(hipMemcpy(out, st.samples.as<float>() + 2u * first, static_cast<size_t>(count) * 2u * sizeof(float), hipMemcpyDeviceToHost));
    return RTX_OK;
}

// ---- the mean of N frames (the kernels: rtx_accum.hip) ---------------------------------------------------------------------

int rtx_accum_add_device(RtxScene *scene, int device, uint32_t n, const void *d_shade, void *d_accum, uint32_t first, void *stream)
{
    if (!scene || !d_shade || !d_accum || !aligned16(d_shade, d_accum)) return RTX_ERR_BAD_ARG;
    if (n == 0u) return RTX_OK;
    Entry e(scene, device, Entry::kCurrent);
    if (e.rc != RTX_OK) return e.rc;
    return hip_rc(rtxc::launch_accum_add(n, d_shade, d_accum, first != 0u, static_cast<hipStream_t>(stream)));
}

int rtx_accum_resolve_device(RtxScene *scene, int device, uint32_t n, const void *d_accum, uint32_t n_frames, void *d_rgb,
                             void *d_shade, void *stream)
{
    if (!scene || !d_accum || (!d_rgb && !d_shade) || !aligned16(d_accum, d_shade)) return RTX_ERR_BAD_ARG;
    if (n_frames == 0u || n_frames > rtx::kMaxMeanFrames) return RTX_ERR_BAD_ARG;
    if (n == 0u) return RTX_OK;
    Entry e(scene, device, Entry::kUploaded);
    if (e.rc != RTX_OK) return e.rc;
    return hip_rc(rtxc::launch_accum_resolve(e.state().thr.as<const float>(), n, d_accum, n_frames, d_rgb, d_shade,
                                             static_cast<hipStream_t>(stream)));
}

int rtx_render_view_mean(RtxScene *scene, int device, const RtxView *view, const RtxLight *light, uint32_t flags,
                         const uint64_t *seeds, uint32_t n_frames, uint32_t n_pairs, uint8_t *out_rgb, RtxPixelShade *out_shade,
                         RtxStats *stats)
{
    MeanCall call;
    const void *out = out_rgb ? static_cast<const void *>(out_rgb) : out_shade;
    if (!mean_args_ok(scene, view, light, flags, seeds, n_frames, n_pairs, out, &call)) return RTX_ERR_BAD_ARG;
    return frames_host(scene, device, view, call, Renderer::kView, nullptr, out_rgb, out_shade, nullptr, stats);
}

int rtx_render_view_mean_device(RtxScene *scene, int device, const RtxView *view, const RtxLight *light, uint32_t flags,
                                const uint64_t *seeds, uint32_t n_frames, uint32_t n_pairs, void *d_accum, void *d_rgb,
                                void *d_shade, void *stream)
{
    MeanCall call;
    if (!d_accum || !aligned16(d_accum, d_shade)) return RTX_ERR_BAD_ARG;
    if (!mean_args_ok(scene, view, light, flags, seeds, n_frames, n_pairs, d_accum, &call)) return RTX_ERR_BAD_ARG;
    return frames_device(scene, device, view, call, Renderer::kView, Sums{nullptr, false, d_accum, nullptr}, d_rgb, d_shade, stream);
}

// ---- the adaptive mean of N frames (the kernels: rtx_adapt.hip) -----------------------------------------------------------------

int rtx_moment_add_device(RtxScene *scene, int device, uint32_t nx, uint32_t ny, const void *d_shade, void *d_moments, void *d_tiles,
                          uint32_t first, const RtxAdaptRule *rule, void *stream)
{
    if (!scene || !d_shade || !d_moments || !aligned16(d_shade, d_moments) || (reinterpret_cast<uintptr_t>(d_tiles) & 7u)) return RTX_ERR_BAD_ARG;
    if ((d_tiles && !rtx::adapt_rule_ok(rule)) || static_cast<uint64_t>(nx) * ny > rtxe::kMaxPixels) return RTX_ERR_BAD_ARG;
    if (nx == 0u || ny == 0u) return RTX_OK;
    Entry e(scene, device, Entry::kCurrent);
    if (e.rc != RTX_OK) return e.rc;
    return hip_rc(rtxe::launch_moment_add(nx, ny, d_shade, d_moments, d_tiles, first != 0u, d_tiles ? *rule : RtxAdaptRule{1u, 0.0f},
                                          static_cast<hipStream_t>(stream)));
}

int rtx_moment_resolve_device(RtxScene *scene, int device, uint32_t n, const void *d_moments, void *d_rgb, void *d_shade, void *stream)
{
    if (!scene || !d_moments || (!d_rgb && !d_shade) || !aligned16(d_moments, d_shade)) return RTX_ERR_BAD_ARG;
    if (n == 0u) return RTX_OK;
    Entry e(scene, device, Entry::kUploaded);
    if (e.rc != RTX_OK) return e.rc;
    return hip_rc(rtxe::launch_moment_resolve(e.state().thr.as<const float>(), n, d_moments, d_rgb, d_shade, static_cast<hipStream_t>(stream)));
}

int rtx_render_view_adaptive(RtxScene *scene, int device, const RtxView *view, const RtxLight *light, uint32_t flags,
                             const uint64_t *seeds, uint32_t n_frames, uint32_t n_pairs, const RtxAdaptRule *rule, uint8_t *out_rgb,
                             RtxPixelShade *out_shade, RtxTileState *out_tiles, RtxStats *stats)
{
    MeanCall call;
    const void *out = out_rgb ? static_cast<const void *>(out_rgb) : out_shade;
    if (!rtx::adapt_rule_ok(rule)) return RTX_ERR_BAD_ARG;
    if (!mean_args_ok(scene, view, light, flags, seeds, n_frames, n_pairs, out, &call)) return RTX_ERR_BAD_ARG;
    return frames_host(scene, device, view, call, Renderer::kMasked, rule, out_rgb, out_shade, out_tiles, stats);
}

int rtx_render_view_adaptive_device(RtxScene *scene, int device, const RtxView *view, const RtxLight *light, uint32_t flags,
                                    const uint64_t *seeds, uint32_t n_frames, uint32_t n_pairs, const RtxAdaptRule *rule,
                                    void *d_moments, void *d_tiles, void *d_rgb, void *d_shade, void *stream)
{
    MeanCall call;
    if (!rtx::adapt_rule_ok(rule) || !d_moments || !d_tiles || !aligned16(d_moments, d_shade) || (reinterpret_cast<uintptr_t>(d_tiles) & 7u))
        return RTX_ERR_BAD_ARG;
    if (!mean_args_ok(scene, view, light, flags & ~RTX_ADAPT_CONTINUE, seeds, n_frames, n_pairs, d_moments, &call)) return RTX_ERR_BAD_ARG;
    return frames_device(scene, device, view, call, Renderer::kMasked, Sums{rule, (flags & RTX_ADAPT_CONTINUE) != 0u, d_moments, d_tiles},
                         d_rgb, d_shade, stream);
}

int rtx_render_view_rows(RtxScene *scene, int device, const RtxView *view, uint8_t *out_rgb, RtxStats *stats)
{
    return view_rows_host(scene, device, view, nullptr, false, out_rgb, stats);
}

int rtx_render_view_rows_device(RtxScene *scene, int device, const RtxView *view, void *d_rgb, size_t d_bytes, void *stream,
                                uint64_t *d_counters)
{
    return view_rows_device(scene, device, view, nullptr, false, d_rgb, d_bytes, stream, d_counters);
}

int rtx_render_view_rows_lit(RtxScene *scene, int device, const RtxView *view, const RtxLight *light, uint8_t *out_rgb,
                             RtxStats *stats)
{
    const CallLight l(scene, light, CallLight::kRequired);
    return l.ok ? view_rows_host(scene, device, view, l.lit, false, out_rgb, stats) : RTX_ERR_BAD_ARG;
}

int rtx_render_view_rows_lit_device(RtxScene *scene, int device, const RtxView *view, const RtxLight *light, void *d_rgb,
                                    size_t d_bytes, void *stream, uint64_t *d_counters)
{
    const CallLight l(scene, light, CallLight::kRequired);
    return l.ok ? view_rows_device(scene, device, view, l.lit, false, d_rgb, d_bytes, stream, d_counters) : RTX_ERR_BAD_ARG;
}

int rtx_scene_light_walk_for(const RtxScene *scene, const RtxLight *light, uint32_t *out_order, float *out_boxes,
                             float *out_shaft_delta)
{
    Lit lit;
    if (!lit_of(scene, light, &lit)) return RTX_ERR_BAD_ARG;
    try {
        light_walk_on_host(scene->prep, lit, out_order, out_boxes, out_shaft_delta);
    } catch (...) {
        return RTX_ERR_OOM;
    }
    return static_cast<int>(scene->prep.nb_ray * lit.count);      // <= 2^20
}

int rtx_debug_light_walk(RtxScene *scene, int device, const RtxLight *light, float *out_tour, float *out_boxes)
{
    Lit lit;
    if (!out_tour || !out_boxes || !lit_of(scene, light, &lit)) return RTX_ERR_BAD_ARG;
    if (!light_is_finite(lit)) return RTX_ERR_UNSUPPORTED;
    Entry e(scene, device, Entry::kUploaded);
    if (e.rc != RTX_OK) return e.rc;
    DeviceState &st = e.state();
    RTX_TRY(reserve_light(scene, st, lit, true));
    RTX_TRY(wait_for_uses(st, kUsesLight));
    RTX_TRY(light_launch(scene, st, lit, true, st.stream));
    const size_t n = static_cast<size_t>(scene->prep.nb_ray) * lit.count;
    if (n) {
        RTX_HIP(hipMemcpyAsync(out_tour, st.lit.tour.as<void>(), n * 4u * sizeof(float), hipMemcpyDeviceToHost, st.stream));
        RTX_HIP(hipMemcpyAsync(out_boxes, st.lit.boxes.as<void>(), static_cast<size_t>(scene->prep.nb_ray) * 6u * sizeof(float),
                               hipMemcpyDeviceToHost, st.stream));
    }
    RTX_HIP(hipStreamSynchronize(st.stream));
    return RTX_OK;
}

int rtx_scene_pose_bound(const RtxScene *scene, float *out)
{
    if (!scene || !out) return RTX_ERR_BAD_ARG;
    *out = scene->prep.scene_magnitude;
    return RTX_OK;
}

int rtx_scene_posed_records(const RtxScene *scene, const float *v0v1v2, const uint32_t *tie_rank, uint32_t *out_tris,
                            uint32_t *out_shade, uint32_t *out_nodes)
{
    if (!scene || !v0v1v2) return RTX_ERR_BAD_ARG;
    return on_host([&] { records_on_host(scene, vertices_alone(v0v1v2, tie_rank, false), nullptr, nullptr, out_tris, out_shade, out_nodes); });
}

int rtx_scene_pose(RtxScene *scene, int device, const float *v0v1v2, const uint32_t *tie_rank, uint32_t reference_tree,
                   RtxStats *stats)
{
    PoseCall call;
    RTX_TRY(vertices_call(scene, v0v1v2, tie_rank, false, true, reference_tree, &call));
    return pose_host(scene, device, call, reference_tree, stats);
}

int rtx_scene_pose_device(RtxScene *scene, int device, const void *d_v0v1v2, const void *d_tie_rank, void *stream)
{
    PoseCall d;
    RTX_TRY(vertices_call(scene, d_v0v1v2, d_tie_rank, false, false, RTX_REFTREE_NEVER, &d));
    return pose_device(scene, device, d, stream);
}

int rtx_scene_pose_rebuilt(RtxScene *scene, int device, const float *v0v1v2, const uint32_t *tie_rank, uint32_t reference_tree,
                           RtxStats *stats)
{
    PoseCall call;
    RTX_TRY(vertices_call(scene, v0v1v2, tie_rank, true, true, reference_tree, &call));
    return pose_host(scene, device, call, reference_tree, stats);
}

int rtx_scene_pose_rebuilt_device(RtxScene *scene, int device, const void *d_v0v1v2, const void *d_tie_rank, void *stream)
{
    PoseCall d;
    RTX_TRY(vertices_call(scene, d_v0v1v2, d_tie_rank, true, false, RTX_REFTREE_NEVER, &d));
    return pose_device(scene, device, d, stream);
}

int rtx_scene_rebuilt_counts(const RtxScene *scene, uint32_t *out_n_nodes)
{
    if (!scene || !out_n_nodes) return RTX_ERR_BAD_ARG;      // (the tables are a cache under the scene's lock)
    return on_host([&] { *out_n_nodes = static_cast<uint32_t>(rebuild_tables_of(const_cast<RtxScene *>(scene)).nodes.size()); });
}

int rtx_scene_rebuilt_records(const RtxScene *scene, const float *v0v1v2, const uint32_t *tie_rank, uint64_t *out_keys,
                              uint32_t *out_perm, uint32_t *out_tris, uint32_t *out_shade, uint32_t *out_nodes)
{
    if (!scene || !v0v1v2) return RTX_ERR_BAD_ARG;
    return on_host([&] { records_on_host(scene, vertices_alone(v0v1v2, tie_rank, true), out_keys, out_perm, out_tris, out_shade, out_nodes); });
}

int rtx_scene_rebuilt_aimed(const RtxScene *scene, const float *v0v1v2, const float eye[3], uint32_t *out_aimed)
{
    if (!scene || !v0v1v2 || !eye || !out_aimed) return RTX_ERR_BAD_ARG;
    return on_host([&] { posed_pipeline_on_host(scene, vertices_alone(v0v1v2, nullptr, true), eye, nullptr, out_aimed); });
}

int rtx_scene_pose_prims(RtxScene *scene, int device, const RtxPosePrims *prims, uint32_t flags, uint32_t reference_tree,
                         RtxStats *stats)
{
    PoseCall call;
    RTX_TRY(prims_call(scene, prims, flags, true, reference_tree, &call));
    return pose_host(scene, device, call, reference_tree, stats);
}

int rtx_scene_pose_prims_device(RtxScene *scene, int device, const RtxPosePrims *prims, uint32_t flags, void *stream)
{
    PoseCall d;
    RTX_TRY(prims_call(scene, prims, flags, false, RTX_REFTREE_NEVER, &d));
    return pose_device(scene, device, d, stream);
}

int rtx_scene_pose_prims_records(const RtxScene *scene, const RtxPosePrims *prims, uint32_t flags, uint64_t *out_keys,
                                 uint32_t *out_perm, uint32_t *out_tris, uint32_t *out_shade, uint32_t *out_nodes)
{
    if (!pose_head_ok(scene, prims, flags)) return RTX_ERR_BAD_ARG;
    if (!(flags & RTX_POSE_REBUILT) && (out_keys || out_perm)) return RTX_ERR_BAD_ARG;
    PoseCall call;
    RTX_TRY(prims_of(scene, prims, flags, &call));
    return on_host([&] { records_on_host(scene, call, out_keys, out_perm, out_tris, out_shade, out_nodes); });
}

int rtx_scene_pose_prims_aimed(const RtxScene *scene, const RtxPosePrims *prims, uint32_t flags, const float eye[3],
                               uint32_t *out_aimed)
{
    if (!pose_head_ok(scene, prims, flags) || !eye || !out_aimed) return RTX_ERR_BAD_ARG;
    PoseCall call;
    RTX_TRY(prims_of(scene, prims, flags, &call));
    call.tie_rank = nullptr;      // (the node words do not depend on it)
    return on_host([&] { posed_pipeline_on_host(scene, call, eye, nullptr, out_aimed); });
}

int rtx_scene_moved_prims(const RtxScene *scene, const RtxPoseMoves *moves, float *out_v0v1v2, float *out_spheres)
{
    if (!scene || !moves) return RTX_ERR_BAD_ARG;
    PoseCall call;
    RTX_TRY(moves_of(scene, moves, 0u, &call));
    rtx::moved_prims(scene->prep, call.moves, out_v0v1v2, out_spheres);
    return RTX_OK;
}

int rtx_scene_pose_moved(RtxScene *scene, int device, const RtxPoseMoves *moves, uint32_t flags, uint32_t reference_tree,
                         RtxStats *stats)
{
    PoseCall call;
    RTX_TRY(moved_call(scene, moves, flags, true, reference_tree, &call));
    return pose_host(scene, device, call, reference_tree, stats);
}

int rtx_scene_pose_moved_device(RtxScene *scene, int device, const RtxPoseMoves *moves, uint32_t flags, void *stream)
{
    PoseCall d;
    RTX_TRY(moved_call(scene, moves, flags, false, RTX_REFTREE_NEVER, &d));
    return pose_device(scene, device, d, stream);
}

int rtx_scene_skin(RtxScene *scene, const RtxSkin *skin)
{
    if (!scene) return RTX_ERR_BAD_ARG;
    if (!skin) {      // unbind: the arrays go, the generation moves on (a device's copy is never taken for a later bind's)
        const uint64_t next = scene->skin.generation + 1u;
        scene->skin = rtx::Skin();
        scene->skin.generation = next;
        return RTX_OK;
    }
    return rtx::skin_bind(scene->prep, skin->bones, skin->weights, skin->sphere_bone, scene->skin);
}

int rtx_scene_skin_bound(const RtxScene *scene, uint32_t *out_max_bone)
{
    if (!scene) return RTX_ERR_BAD_ARG;
    if (out_max_bone) *out_max_bone = scene->skin.bound ? scene->skin.max_bone : 0u;
    return scene->skin.bound ? 1 : 0;
}

int rtx_scene_skinned_prims(const RtxScene *scene, const RtxPoseMoves *moves, float *out_v0v1v2, float *out_spheres)
{
    if (!scene || !moves) return RTX_ERR_BAD_ARG;
    PoseCall call;
    RTX_TRY(moves_of(scene, moves, 0u, &call));
    if (call.moves.group || !scene->skin.bound) return RTX_ERR_BAD_ARG;
    rtx::skinned_prims(scene->prep, scene->skin, call.moves, out_v0v1v2, out_spheres);
    return RTX_OK;
}

int rtx_scene_pose_skinned(RtxScene *scene, int device, const RtxPoseMoves *moves, uint32_t flags, uint32_t reference_tree,
                           RtxStats *stats)
{
    PoseCall call;
    RTX_TRY(skinned_call(scene, moves, flags, true, reference_tree, &call));
    return pose_host(scene, device, call, reference_tree, stats);
}

int rtx_scene_pose_skinned_device(RtxScene *scene, int device, const RtxPoseMoves *moves, uint32_t flags, void *stream)
{
    PoseCall d;
    RTX_TRY(skinned_call(scene, moves, flags, false, RTX_REFTREE_NEVER, &d));
    return pose_device(scene, device, d, stream);
}

int rtx_debug_moved_prims(RtxScene *scene, int device, float *out_v0v1v2, float *out_spheres)
{
    if (!scene) return RTX_ERR_BAD_ARG;
    Entry e(scene, device, Entry::kUploaded);
    if (e.rc != RTX_OK) return e.rc;
    DeviceState &st = e.state();
    if (!st.pose.f.ran) return RTX_ERR_BAD_ARG;
    const size_t v_bytes = scene->prep.rest_v0v1v2.size() * sizeof(float), s_bytes = scene->prep.rest_spheres.size() * sizeof(float);
    RTX_TRY(wait_for_uses(st, kUsesPose));
    if (out_v0v1v2 && v_bytes) RTX_HIP(hipMemcpyAsync(out_v0v1v2, st.pose.v.as<void>(), v_bytes, hipMemcpyDeviceToHost, st.stream));
    if (out_spheres && s_bytes)
        RTX_HIP(hipMemcpyAsync(out_spheres, st.pose.m.spheres.as<void>(), s_bytes, hipMemcpyDeviceToHost, st.stream));
    return read_back_nodes(st, nullptr, 0u, nullptr);
}

int rtx_debug_pose_rebuilt(RtxScene *scene, int device, const float eye[3], uint32_t *out_perm, uint32_t *out_tris,
                           uint32_t *out_shade, uint32_t *out_nodes, uint32_t *out_aimed)
{
    return debug_pose(scene, device, true, eye, out_perm, out_tris, out_shade, out_nodes, out_aimed);
}

int rtx_debug_pose(RtxScene *scene, int device, uint32_t *out_tris, uint32_t *out_shade, uint32_t *out_nodes)
{
    return debug_pose(scene, device, false, nullptr, nullptr, out_tris, out_shade, out_nodes, nullptr);
}

int rtx_trace_rays_posed(RtxScene *scene, int device, uint32_t n_rays, const float *origins, const float *directions,
                         uint32_t flags, RtxRayHit *out_hits, RtxStats *stats)
{
    if (!query_args_ok(scene, origins, directions, out_hits, flags, n_rays)) return RTX_ERR_BAD_ARG;
    return batch_host(scene, device, query_batch(false, n_rays, flags, true), origins, directions, {out_hits, nullptr, nullptr}, stats);
}

int rtx_occluded_rays_posed(RtxScene *scene, int device, uint32_t n_rays, const float *origins, const float *targets,
                            uint32_t flags, uint8_t *out_occluded, RtxStats *stats)
{
    if (!query_args_ok(scene, origins, targets, out_occluded, flags, n_rays)) return RTX_ERR_BAD_ARG;
    return batch_host(scene, device, query_batch(true, n_rays, flags, true), origins, targets, {out_occluded, nullptr, nullptr}, stats);
}

int rtx_trace_rays_posed_device(RtxScene *scene, int device, uint32_t n_rays, const void *d_origins, const void *d_directions,
                                uint32_t flags, void *d_hits, void *stream)
{
    if (!query_args_ok(scene, d_origins, d_directions, d_hits, flags, n_rays) || !aligned16(d_hits)) return RTX_ERR_BAD_ARG;
    return batch_device(scene, device, query_batch(false, n_rays, flags, true), d_origins, d_directions, {d_hits, nullptr, nullptr}, stream);
}

int rtx_occluded_rays_posed_device(RtxScene *scene, int device, uint32_t n_rays, const void *d_origins, const void *d_targets,
                                   uint32_t flags, void *d_occluded, void *stream)
{
    if (!query_args_ok(scene, d_origins, d_targets, d_occluded, flags, n_rays)) return RTX_ERR_BAD_ARG;
    return batch_device(scene, device, query_batch(true, n_rays, flags, true), d_origins, d_targets, {d_occluded, nullptr, nullptr}, stream);
}

int rtx_shade_rays_posed(RtxScene *scene, int device, uint32_t n_pixels, const float *origins, const float *directions,
                         uint32_t flags, const RtxLight *light, RtxPixelShade *out_shade, RtxRayHit *out_hits, RtxStats *stats)
{
    const CallLight l(scene, light, CallLight::kOptional);
    return l.ok ? shade_host(scene, device, n_pixels, origins, directions, flags, l.lit, true, out_shade, out_hits, stats) : RTX_ERR_BAD_ARG;
}

int rtx_shade_rays_posed_device(RtxScene *scene, int device, uint32_t n_pixels, const void *d_origins, const void *d_directions,
                                uint32_t flags, const RtxLight *light, void *d_shade, void *d_hits, void *stream)
{
    const CallLight l(scene, light, CallLight::kOptional);
    return l.ok ? shade_device(scene, device, n_pixels, d_origins, d_directions, flags, l.lit, true, d_shade, d_hits, stream) : RTX_ERR_BAD_ARG;
}

int rtx_render_view_posed(RtxScene *scene, int device, const RtxView *view, const RtxLight *light, uint8_t *out_rgb,
                          RtxPixelShade *out_shade, RtxRayHit *out_hits, RtxStats *stats)
{
    const CallLight l(scene, light, CallLight::kOptional);
    return l.ok ? view_host(scene, device, view, l.lit, true, out_rgb, out_shade, out_hits, stats) : RTX_ERR_BAD_ARG;
}

int rtx_render_view_posed_device(RtxScene *scene, int device, const RtxView *view, const RtxLight *light, void *d_rgb,
                                 void *d_shade, void *d_hits, void *stream)
{
    const CallLight l(scene, light, CallLight::kOptional);
    return l.ok ? view_device(scene, device, view, l.lit, true, d_rgb, d_shade, d_hits, stream) : RTX_ERR_BAD_ARG;
}

int rtx_scene_aimed_nodes(const RtxScene *scene, const float eye[3], uint32_t *out_dwords)
{
    if (!scene || !eye || !out_dwords) return RTX_ERR_BAD_ARG;
    try {
        const std::vector<rtx::NodeRec> v = aimed_on_host(scene->prep, eye);
        std::memcpy(out_dwords, v.data(), v.size() * sizeof(rtx::NodeRec));
    } catch (...) {
        return RTX_ERR_OOM;
    }
    return RTX_OK;
}

int rtx_debug_aimed_nodes(RtxScene *scene, int device, const float eye[3], uint32_t *out_dwords)
{
    if (!scene || !eye || !out_dwords) return RTX_ERR_BAD_ARG;
    Entry e(scene, device, Entry::kUploaded);
    if (e.rc != RTX_OK) return e.rc;
    DeviceState &st = e.state();
    int rc = reserve_aimed(scene, st.geo);
    if (rc != RTX_OK) return rc;
    st.geo.aimed.valid = false;              // the kernels run whatever the buffer holds
    if ((rc = aim_at(scene, st.geo, eye, st.stream)) != RTX_OK) return rc;
    return read_back_nodes(st, aimed_stream(scene, st.geo), scene->prep.nodes.size(), out_dwords);
}

int rtx_render_view_rows_posed(RtxScene *scene, int device, const RtxView *view, const RtxLight *light, uint8_t *out_rgb,
                               RtxStats *stats)
{
    const CallLight l(scene, light, CallLight::kOptional);
    return l.ok ? view_rows_host(scene, device, view, l.lit, true, out_rgb, stats) : RTX_ERR_BAD_ARG;
}

int rtx_render_view_rows_posed_device(RtxScene *scene, int device, const RtxView *view, const RtxLight *light, void *d_rgb,
                                      size_t d_bytes, void *stream, uint64_t *d_counters)
{
    const CallLight l(scene, light, CallLight::kOptional);
    return l.ok ? view_rows_device(scene, device, view, l.lit, true, d_rgb, d_bytes, stream, d_counters) : RTX_ERR_BAD_ARG;
}

// The pipeline's records: view_rows_host / view_rows_device with the light (NULL: the scene's, nothing swapped) and the
// geometry (RTX_ROWS_POSED) as arguments, as the byte calls are inside this file.
int rtx_render_view_rows_shade(RtxScene *scene, int device, const RtxView *view, const RtxLight *light, uint32_t flags,
                               RtxPixelShade *out_shade, RtxStats *stats)
{
    if (flags & ~RTX_ROWS_POSED) return RTX_ERR_BAD_ARG;
    const CallLight l(scene, light, CallLight::kOptional);
    return l.ok ? view_rows_host(scene, device, view, l.lit, (flags & RTX_ROWS_POSED) != 0u, out_shade, stats, true) : RTX_ERR_BAD_ARG;
}

int rtx_render_view_rows_shade_device(RtxScene *scene, int device, const RtxView *view, const RtxLight *light, uint32_t flags,
                                      void *d_shade, size_t d_bytes, void *stream, uint64_t *d_counters)
{
    if (flags & ~RTX_ROWS_POSED) return RTX_ERR_BAD_ARG;
    const CallLight l(scene, light, CallLight::kOptional);
    return l.ok ? view_rows_device(scene, device, view, l.lit, (flags & RTX_ROWS_POSED) != 0u, d_shade, d_bytes, stream, d_counters, true)
                : RTX_ERR_BAD_ARG;
}

// The pipeline's records behind a tile mask: rtx_render_view_rows_shade_device with the states and the rule as arguments.
int rtx_render_view_rows_shade_masked_device(RtxScene *scene, int device, const RtxView *view, const RtxLight *light, uint32_t flags,
                                             const void *d_tiles, const RtxAdaptRule *rule, void *d_shade, size_t d_bytes, void *stream,
                                             uint64_t *d_counters)
{
    if (flags & ~RTX_ROWS_POSED) return RTX_ERR_BAD_ARG;
    const CallLight l(scene, light, CallLight::kOptional);
    if (!l.ok || !d_tiles || (reinterpret_cast<uintptr_t>(d_tiles) & 7u) || !rtx::adapt_rule_ok(rule)) return RTX_ERR_BAD_ARG;
    const TileMask mask{d_tiles, *rule};
    return view_rows_device(scene, device, view, l.lit, (flags & RTX_ROWS_POSED) != 0u, d_shade, d_bytes, stream, d_counters, true, &mask);
}

int rtx_render_view_rows_mean(RtxScene *scene, int device, const RtxView *view, const RtxLight *light, uint32_t flags,
                              const uint64_t *seeds, uint32_t n_frames, uint32_t n_pairs, uint8_t *out_rgb, RtxPixelShade *out_shade,
                              RtxStats *stats)
{
    MeanCall call;
    const void *out = out_rgb ? static_cast<const void *>(out_rgb) : out_shade;
    if (!mean_args_ok(scene, view, light, flags, seeds, n_frames, n_pairs, out, &call)) return RTX_ERR_BAD_ARG;
    return frames_host(scene, device, view, call, Renderer::kRows, nullptr, out_rgb, out_shade, nullptr, stats);
}

int rtx_render_view_rows_mean_device(RtxScene *scene, int device, const RtxView *view, const RtxLight *light, uint32_t flags,
                                     const uint64_t *seeds, uint32_t n_frames, uint32_t n_pairs, void *d_accum, void *d_rgb,
                                     void *d_shade, void *stream)
{
    MeanCall call;
    if (!d_accum || !aligned16(d_accum, d_shade)) return RTX_ERR_BAD_ARG;
    if (!mean_args_ok(scene, view, light, flags, seeds, n_frames, n_pairs, d_accum, &call)) return RTX_ERR_BAD_ARG;
    return frames_device(scene, device, view, call, Renderer::kRows, Sums{nullptr, false, d_accum, nullptr}, d_rgb, d_shade, stream);
}

// The adaptive mean through the pipeline: rtx_render_view_adaptive's checks, then the pipeline's (frames_refused).
int rtx_render_view_rows_adaptive(RtxScene *scene, int device, const RtxView *view, const RtxLight *light, uint32_t flags,
                                  const uint64_t *seeds, uint32_t n_frames, uint32_t n_pairs, const RtxAdaptRule *rule, uint8_t *out_rgb,
                                  RtxPixelShade *out_shade, RtxTileState *out_tiles, RtxStats *stats)
{
    MeanCall call;
    const void *out = out_rgb ? static_cast<const void *>(out_rgb) : out_shade;
    if (!rtx::adapt_rule_ok(rule)) return RTX_ERR_BAD_ARG;
    if (!mean_args_ok(scene, view, light, flags, seeds, n_frames, n_pairs, out, &call)) return RTX_ERR_BAD_ARG;
    return frames_host(scene, device, view, call, Renderer::kRowsMasked, rule, out_rgb, out_shade, out_tiles, stats);
}

int rtx_render_view_rows_adaptive_device(RtxScene *scene, int device, const RtxView *view, const RtxLight *light, uint32_t flags,
                                         const uint64_t *seeds, uint32_t n_frames, uint32_t n_pairs, const RtxAdaptRule *rule,
                                         void *d_moments, void *d_tiles, void *d_rgb, void *d_shade, void *stream)
{
    MeanCall call;
    if (!rtx::adapt_rule_ok(rule) || !d_moments || !d_tiles || !aligned16(d_moments, d_shade) || (reinterpret_cast<uintptr_t>(d_tiles) & 7u))
        return RTX_ERR_BAD_ARG;
    if (!mean_args_ok(scene, view, light, flags & ~RTX_ADAPT_CONTINUE, seeds, n_frames, n_pairs, d_moments, &call)) return RTX_ERR_BAD_ARG;
    return frames_device(scene, device, view, call, Renderer::kRowsMasked, Sums{rule, (flags & RTX_ADAPT_CONTINUE) != 0u, d_moments, d_tiles},
                         d_rgb, d_shade, stream);
}

int rtx_scene_light_walk_seeded(const RtxScene *scene, const RtxLight *light, uint64_t seed, uint32_t n_pairs, uint32_t *out_order,
                                float *out_boxes, float *out_shaft_delta)
{
    if (!scene || n_pairs == 0u) return RTX_ERR_BAD_ARG;
    RtxLight own;
    if (!light && rtx_scene_light(scene, &own) != RTX_OK) return RTX_ERR_BAD_ARG;
    Lit lit;
    if (!lit_of(scene, light ? light : &own, &lit)) return RTX_ERR_BAD_ARG;
    try {
        light_walk_on_host(scene->prep, lit, rtx::SampleSource{nullptr, seed, n_pairs}, out_order, out_boxes, out_shaft_delta);
    } catch (...) {
        return RTX_ERR_OOM;
    }
    return static_cast<int>(scene->prep.nb_ray * lit.count);      // <= 2^20
}

int rtx_scene_posed_pipeline_records(const RtxScene *scene, const float *v0v1v2, const float eye[3], uint32_t *out_planes,
                                     uint32_t *out_aimed)
{
    if (!scene || !v0v1v2 || (out_aimed && !eye)) return RTX_ERR_BAD_ARG;
    return on_host([&] { posed_pipeline_on_host(scene, vertices_alone(v0v1v2, nullptr, false), eye, out_planes, out_aimed); });
}

int rtx_debug_pose_pipeline(RtxScene *scene, int device, const float eye[3], uint32_t *out_planes, uint32_t *out_aimed)
{
    if (!scene || (out_aimed && !eye)) return RTX_ERR_BAD_ARG;
    Entry e(scene, device, Entry::kUploaded);
    if (e.rc != RTX_OK) return e.rc;
    DeviceState &st = e.state();
    DeviceGeometry *g;
    RTX_TRY(geometry_of(st, true, &g));
    if (st.pose.rebuilt && out_aimed) return RTX_ERR_BAD_ARG;      // sized by the uploaded node count: rtx_debug_pose_rebuilt
    const size_t n = scene->prep.nodes.size(), n_global = scene->prep.n_global;
    RTX_TRY(wait_for_uses(st, kUsesPose));
    if (out_planes && n_global)
        RTX_HIP(hipMemcpyAsync(out_planes, g->planes.as<void>(), n_global * sizeof(rtx::TriRec), hipMemcpyDeviceToHost, st.stream));
    return read_back_aimed(scene, st, *g, eye, n, out_aimed);
}

int rtx_debug_wave_profile(RtxScene *scene, int device, uint32_t row0, uint32_t nrows, uint64_t *out,
                           size_t out_tiles, uint32_t *tiles_x, uint32_t *tiles_y)
{
    if (!scene || !tiles_x || !tiles_y) return RTX_ERR_BAD_ARG;
    const uint32_t H = scene->prep.height;
    if (row0 > H || nrows > H - row0 || nrows == 0) return RTX_ERR_BAD_ARG;
#if !RTX_ABLATION
    // the per-tile instrumentation lives in the fused kernel, which only librtx_ablation.so carries
    (void)device; (void)out; (void)out_tiles;
    return RTX_ERR_UNSUPPORTED;
#else
    Entry en(scene, device, Entry::kUploaded);
    if (en.rc != RTX_OK) return en.rc;
    DeviceState &st = en.state();
    const rtx::DeviceScene S = device_scene(scene, st, st.geo);
    *tiles_x = rtx::trace_tiles_x(S, kernel_variant());
    *tiles_y = (nrows + 7u) / 8u;
    const size_t n = static_cast<size_t>(*tiles_x) * *tiles_y;
    if (!out) return RTX_OK;   // size query
    if (out_tiles < n) return RTX_ERR_BAD_ARG;
    int rc = st.d_out.reserve(static_cast<size_t>(nrows) * scene->prep.width * 3u);
    if (rc != RTX_OK) return rc;
    unsigned long long *d_prof = nullptr;
    const size_t prof_bytes = n * rtx::kWaveProfWords * sizeof(unsigned long long);
    RTX_HIP(hipMalloc(reinterpret_cast<void **>(&d_prof), prof_bytes));
    const rtx::TileSpec ts{row0, nrows, nrows, nrows};
    rc = render_launch(st, S, ts, st.d_out.as<uint8_t>(), nullptr, d_prof, st.stream,
                       [&] { return hip_rc(hipMemsetAsync(d_prof, 0, prof_bytes, st.stream)); });
    if (rc == RTX_OK) rc = hip_rc(hipMemcpyAsync(out, d_prof, prof_bytes, hipMemcpyDeviceToHost, st.stream));
    if (rc == RTX_OK) rc = hip_rc(hipStreamSynchronize(st.stream));
    (void)hipFree(d_prof);
    if (rc != RTX_OK) return rc;
    for (size_t t = 0; t < n; ++t)   // the kernel keeps the earliest start as max(~t)
        out[rtx::kWaveProfWords * t + 2] = ~out[rtx::kWaveProfWords * t + 2];
    return RTX_OK;
#endif
}

int rtx_debug_tile_descs(RtxScene *scene, int device, uint32_t *out, size_t max_tiles)
{
    if (!scene) return RTX_ERR_BAD_ARG;
    Entry e(scene, device, Entry::kLocked);
    if (e.rc != RTX_OK) return e.rc;
    const DeviceState &st = e.state();
    if (!out) return static_cast<int>(st.last_tiles);      // (answered without making the device current)
    const int rc = e.make_current();
    if (rc != RTX_OK) return rc;
    const size_t n = st.last_tiles < max_tiles ? st.last_tiles : max_tiles;
    RTX_HIP(hipDeviceSynchronize());
    if (n) RTX_HIP(hipMemcpy(out, st.ws.tiles.as<void>(), n * sizeof(rtx::TileDesc), hipMemcpyDeviceToHost));
    return static_cast<int>(n);
}

int rtx_debug_probe_records(RtxScene *scene, int device, uint32_t *out_hits, uint32_t *out_pix_slots, size_t max_tiles)
{
    if (!scene) return RTX_ERR_BAD_ARG;
    Entry e(scene, device, Entry::kLocked);
    if (e.rc != RTX_OK) return e.rc;
    const DeviceState &st = e.state();
    if (!out_hits && !out_pix_slots) return static_cast<int>(st.last_tiles);
    const int rc = e.make_current();
    if (rc != RTX_OK) return rc;
    const size_t n = st.last_tiles < max_tiles ? st.last_tiles : max_tiles;
    RTX_HIP(hipDeviceSynchronize());
    if (n && out_hits) RTX_HIP(hipMemcpy(out_hits, st.ws.hits.as<void>(), n * 64u * sizeof(rtx::HitRec), hipMemcpyDeviceToHost));
    if (n && out_pix_slots) RTX_HIP(hipMemcpy(out_pix_slots, st.ws.pix_slot.as<void>(), n * 64u * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return static_cast<int>(n);
}

int rtx_debug_probe_split(RtxScene *scene, uint32_t mode)
{
    if (!scene || mode > 2u) return RTX_ERR_BAD_ARG;
    scene->split_mode = mode;
    return static_cast<int>(scene->last_long.load());
}

int rtx_scene_probe_long(const RtxScene *scene, uint32_t *out_tiles, uint32_t *out_weights, size_t max_entries, uint32_t *out_threshold)
{
    if (!scene) return RTX_ERR_BAD_ARG;
    const rtx::PreparedScene &p = scene->prep;
    const size_t n = p.long_tiles.size() < max_entries ? p.long_tiles.size() : max_entries;
    if (out_tiles && n) std::memcpy(out_tiles, p.long_tiles.data(), n * sizeof(uint32_t));
    if (out_weights && n) std::memcpy(out_weights, p.long_weights.data(), n * sizeof(uint32_t));
    if (out_threshold) *out_threshold = rtx::kProbeLongWeight;
    return static_cast<int>(out_tiles || out_weights ? n : p.long_tiles.size());
}

int rtx_scene_probe_tile(const RtxScene *scene, uint32_t tile_x, uint32_t tile_y, uint8_t *out_met, uint32_t *out_weight)
{
    if (!scene || !out_weight) return RTX_ERR_BAD_ARG;
    const rtx::PreparedScene &p = scene->prep;
    if (tile_x >= (p.width + 7u) / 8u || tile_y >= (p.height + 7u) / 8u) return RTX_ERR_BAD_ARG;
    if (out_met) std::memset(out_met, 0, p.nodes.size());
    bool valid = false;
    *out_weight = rtx::probe_tile_weight(p, tile_x, tile_y, out_met, &valid);
    return valid ? 1 : 0;
}

int rtx_launch_timings(RtxScene *scene, int device, int max_launches, float *schedule_ms, float *shade_ms)
{
    if (!scene || max_launches < 0 || !schedule_ms || !shade_ms) return RTX_ERR_BAD_ARG;
    Entry e(scene, device, Entry::kCurrent);
    if (e.rc != RTX_OK) return e.rc;
    const DeviceState &st = e.state();
    unsigned long long n = st.launches < RTX_TIMING_RING ? st.launches : RTX_TIMING_RING;
    if (n > static_cast<unsigned long long>(max_launches)) n = static_cast<unsigned long long>(max_launches);
    for (unsigned long long i = 0; i < n; ++i) {
        const Event *ev = st.ring[(st.launches - n + i) % RTX_TIMING_RING];
        RTX_HIP(hipEventSynchronize(ev[2]));
        RTX_HIP(hipEventElapsedTime(&schedule_ms[i], ev[0], ev[1]));
        RTX_HIP(hipEventElapsedTime(&shade_ms[i], ev[1], ev[2]));
    }
    return static_cast<int>(n);
}

int rtx_scene_light_points(const RtxScene *scene, float *out)
{
    if (!scene || !out) return RTX_ERR_BAD_ARG;
    std::memcpy(out, scene->prep.light_points.data(), scene->prep.light_points.size() * sizeof(float));
    return RTX_OK;
}

int rtx_scene_light_order(const RtxScene *scene, uint32_t *out)
{
    if (!scene || !out) return RTX_ERR_BAD_ARG;
    std::memcpy(out, scene->prep.light_order.data(), scene->prep.light_order.size() * sizeof(uint32_t));
    return RTX_OK;
}

int rtx_scene_gamma_thresholds(const RtxScene *scene, float *out256)
{
    if (!scene || !out256) return RTX_ERR_BAD_ARG;
    std::memcpy(out256, scene->prep.gamma_thr, sizeof scene->prep.gamma_thr);
    return RTX_OK;
}

int rtx_scene_normals(const RtxScene *scene, float *out)
{
    if (!scene || !out) return RTX_ERR_BAD_ARG;
    for (size_t i = 0; i < scene->prep.shade.size(); ++i) std::memcpy(out + 3 * i, scene->prep.shade[i].normal, 12);
    return RTX_OK;
}

int rtx_scene_ref_nodes(const RtxScene *scene, uint32_t *out_dwords)
{
    if (!scene || !out_dwords) return RTX_ERR_BAD_ARG;
    std::memcpy(out_dwords, scene->prep.ref_nodes.data(), scene->prep.ref_nodes.size() * sizeof(rtx::NodeRec));
    return RTX_OK;
}

int rtx_scene_primary_nodes(const RtxScene *scene, uint32_t *out_dwords, uint32_t *out_own)
{
    if (!scene) return RTX_ERR_BAD_ARG;
    const bool own = !scene->prep.primary_nodes.empty();
    const std::vector<rtx::NodeRec> &v = own ? scene->prep.primary_nodes : scene->prep.nodes;
    if (out_dwords) std::memcpy(out_dwords, v.data(), v.size() * sizeof(rtx::NodeRec));
    if (out_own) *out_own = own ? 1u : 0u;
    return RTX_OK;
}

int rtx_scene_nodes(const RtxScene *scene, uint32_t *out_dwords, uint32_t *out_tri_order)
{
    if (!scene) return RTX_ERR_BAD_ARG;
    if (out_dwords)
        std::memcpy(out_dwords, scene->prep.nodes.data(), scene->prep.nodes.size() * sizeof(rtx::NodeRec));
    if (out_tri_order)
        for (size_t i = 0; i < scene->prep.tris.size(); ++i) out_tri_order[i] = scene->prep.tris[i].idx;
    return RTX_OK;
}

}  // extern "C"
