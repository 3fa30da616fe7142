// host_pass.h -- how a post pass hangs off a frame, said once: what the accumulation, the ambient obscurance, the depth of
// field, the motion blur and the per-face velocity share on the host.  The weak launches of their code objects, the
// timing marks round a pass's kernels, the record a scene keeps of a pass, the staged table a frame slot uploads, the
// device buffers of a debug entry, and the checks every description and mirror makes.  Nothing here belongs to one pass:
// the description, the kernel launch, the mirror and the debug entry of each are in its own header.
//
// It stands in front of host_scene.h, because mr_scene holds the records by value.
#pragma once

// ---- the launches of accum.hip, ao.hip, dof.hip, motion.hip, motion_faces.hip, taa.hip, bloom.hip, shafts.hip, tonemap.hip and layers.hip, the library's other translation units,
// each declared here and nowhere else; weak, so that a library linked without one of them (the tools' ablation builds)
// still loads: it refuses that pass instead (linked)
namespace mr_accum {
__attribute__((weak)) void launch_add(hipStream_t stream, const float *frame, float *acc, size_t n_floats, float w, int first);
__attribute__((weak)) void launch_resolve(hipStream_t stream, const float *acc, int width, int height, int shift, float scale,
                                          const float *gamma_lut, uint8_t *out);
}  // namespace mr_accum
namespace mr_ao {
__attribute__((weak)) void launch(hipStream_t stream, const double *zbuf, float *frame, int width, int height, const mr::AoParams &p,
                                  int shape);
}  // namespace mr_ao
namespace mr_dof {
__attribute__((weak)) void launch(hipStream_t stream, const double *zbuf, const float *frame, float *out, int width, int height,
                                  const mr::DofParams &p, int shape);
}  // namespace mr_dof
namespace mr_motion {
__attribute__((weak)) void launch_velocity(hipStream_t stream, const double *zbuf, const int32_t *winner, const double *tables, float *vel,
                                           int width, int height, const mr::MotionParams &p);
__attribute__((weak)) void launch_blur(hipStream_t stream, const double *zbuf, const float *vel, const float *frame, float *out, int width,
                                       int height, const mr::MotionParams &p, int shape);
}  // namespace mr_motion
namespace mr_motion_faces {
__attribute__((weak)) void launch_homography(hipStream_t stream, const int32_t *faces, const double *verts, const double *verts_prev,
                                             const int32_t *tables, double *hom, const mr::MotionFacesParams &p);
__attribute__((weak)) void launch_velocity_faces(hipStream_t stream, const int32_t *winner, const int32_t *tables, const double *hom, float *vel,
                                                 int width, int height, int n_models);
}  // namespace mr_motion_faces
namespace mr_taa {
__attribute__((weak)) void launch(hipStream_t stream, const float *frame, const float *vel, const float *hist, float *out, float *hist_out,
                                  int width, int height, const mr::TaaParams &p, int shape);
}  // namespace mr_taa
namespace mr_bloom {
__attribute__((weak)) void launch_down(hipStream_t stream, const float *src, float *dst, int sw, int sh, float threshold, int first, int shape);
__attribute__((weak)) void launch_up(hipStream_t stream, float *fine, const float *coarse, int w, int h);
__attribute__((weak)) void launch_composite(hipStream_t stream, float *frame, const float *coarse, int w, int h, float gain);
}  // namespace mr_bloom
namespace mr_shafts {
__attribute__((weak)) void launch_source(hipStream_t stream, const float *frame, const double *zbuf, float *dst, int w, int h, int dw, int dh,
                                         float threshold, int levels);
__attribute__((weak)) void launch_march(hipStream_t stream, const float *src, float *dst, int w, int h, const mr::ShaftsParams &p);
__attribute__((weak)) void launch_composite(hipStream_t stream, float *frame, const float *coarse, int w, int h, int cw, int ch, int levels, float gain);
}  // namespace mr_shafts
namespace mr_tonemap {
__attribute__((weak)) unsigned hist_grid(size_t n_samples, unsigned cap);
__attribute__((weak)) void launch_hist(hipStream_t stream, const float *frame, size_t n_samples, uint32_t *slab, unsigned grid, int form);
__attribute__((weak)) void launch_exposure(hipStream_t stream, const uint32_t *slab, unsigned rows, const mr::ToneMeter &meter, const float *e_prev,
                                           uint32_t *hist, float *e_cell, float *e_next);
__attribute__((weak)) void launch_apply(hipStream_t stream, float *frame, size_t n_floats, int op, const float *e_cell, float e_fixed, float white2);
}  // namespace mr_tonemap
namespace mr_layers {
__attribute__((weak)) void launch(hipStream_t stream, const mr::LayersArgs &a, const mr::LayersParams &p, int pos32);
}  // namespace mr_layers

namespace {

// MR_OK when every one of these launches was linked in; else the pass's refusal
template <class... Launch>
inline int linked(const char *refusal, Launch *...launch)
{
    if ((... && (launch != nullptr))) return MR_OK;
    return fail(MR_E_UNSUPPORTED, refusal);
}

// k_taa is taa.hip's; its velocity is motion.hip's k_velocity; the bytes of such a frame are the accumulation's resolve of
// its float frame (accum.hip)
inline int taa_linked()
{
    return linked("this library was linked without taa.hip, motion.hip or accum.hip: no temporal anti-aliasing (build it with __graft_entry__.build())",
                  &mr_taa::launch, &mr_motion::launch_velocity, &mr_accum::launch_resolve);
}

// the bloom's three kernels are bloom.hip's; the bytes of a bloomed frame are the accumulation's resolve of its float frame
// (accum.hip)
inline int bloom_linked()
{
    return linked("this library was linked without bloom.hip or accum.hip: no bloom (build it with __graft_entry__.build())",
                  &mr_bloom::launch_down, &mr_bloom::launch_up, &mr_bloom::launch_composite, &mr_accum::launch_resolve);
}

// the light shafts' three kernels are shafts.hip's; the bytes of such a frame are the accumulation's resolve of its float
// frame (accum.hip)
inline int shafts_linked()
{
    return linked("this library was linked without shafts.hip or accum.hip: no light shafts (build it with __graft_entry__.build())",
                  &mr_shafts::launch_source, &mr_shafts::launch_march, &mr_shafts::launch_composite, &mr_accum::launch_resolve);
}

// the tone mapping's three kernels are tonemap.hip's; the bytes of such a frame are the accumulation's resolve of its float
// frame (accum.hip)
inline int tonemap_linked()
{
    return linked("this library was linked without tonemap.hip or accum.hip: no tone mapping (build it with __graft_entry__.build())",
                  &mr_tonemap::hist_grid, &mr_tonemap::launch_hist, &mr_tonemap::launch_exposure, &mr_tonemap::launch_apply, &mr_accum::launch_resolve);
}

// ---- timing marks: N events round a pass's kernels, created by the first frame that records them and kept for the
// scene's life.  An event that exists is not null: that is the one rule of create() and release().
template <int N>
struct Marks {
    hipEvent_t ev[N] = {};
    int create()
    {
        for (hipEvent_t &e : ev)
            if (!e) HIP_TRY(hipEventCreate(&e));
        return MR_OK;
    }
    int record(int i, hipStream_t stream) const
    {
        HIP_TRY(hipEventRecord(ev[i], stream));
        return MR_OK;
    }
    // device milliseconds between two marks, for the mr_debug_*_times entries: no entry point waits for a pass's kernels,
    // so this waits for the later mark first
    int elapsed(int from, int to, float *out_ms) const
    {
        HIP_TRY(hipEventSynchronize(ev[to]));
        HIP_TRY(hipEventElapsedTime(out_ms, ev[from], ev[to]));
        return MR_OK;
    }
    void release()
    {
        for (hipEvent_t &e : ev) {
            if (e) (void)hipEventDestroy(e);
            e = nullptr;
        }
    }
};

// What a scene keeps of a pass that runs behind a frame's tile kernel; mr_scene::Ao, Dof and Motion are this and the
// description every frame enqueued from now on takes a copy of (params).  The marks are the scene's, not a slot's: they
// stand round the pass of the LAST frame enqueued, whatever other frames are in flight (diagnostics only).
template <int N>
struct PassRecord {
    bool on = false;
    int32_t frames = 0, rows = 0, cols = 0;            // frames that enqueued the pass; the last one's sample grid
    Marks<N> marks;                                    // [0] in front of the pass's first kernel, [N - 1] behind its last
    bool marked = false;
};

// A pass on a frame's stream: mark 0, what `launch` enqueues (it records the marks in between), mark N - 1, and the
// record's counters.
template <int N, class Launch>
int marked_launch(PassRecord<N> &a, hipStream_t stream, int width, int height, Launch &&launch)
{
    if (int rc = a.marks.create()) return rc;
    if (int rc = a.marks.record(0, stream)) return rc;
    if (int rc = launch()) return rc;
    if (int rc = a.marks.record(N - 1, stream)) return rc;
    a.marked = true;
    a.frames += 1; a.rows = height; a.cols = width;
    return MR_OK;
}

// the scene lets go of a pass (or of the accumulation): its events destroyed, everything else as a new scene has it
template <class Pass>
void release_pass(Pass &a)
{
    a.marks.release();
    a = Pass();
}

// ---- A table a frame slot uploads for a pass: its device copy and the page-locked copy the upload reads, with an event
// behind the upload -- the host waits for it before it writes the next frame's table there (a frame in flight on the
// slot's stream keeps its own device copy until then; frames on other streams have other slots).
struct StagedTable {
    DevBuf d_tables;
    void *h_tables = nullptr;
    size_t h_cap = 0;
    hipEvent_t copied = nullptr;
    bool pending = false;
    int stage(const void *from, size_t bytes, hipStream_t stream)
    {
        if (!copied) HIP_TRY(hipEventCreateWithFlags(&copied, hipEventDisableTiming));
        if (pending) { HIP_TRY(hipEventSynchronize(copied)); pending = false; }
        if (bytes > h_cap) {
            if (h_tables) HIP_TRY(hipHostFree(h_tables));
            h_tables = nullptr; h_cap = 0;
            HIP_TRY(hipHostMalloc(&h_tables, bytes * 2, hipHostMallocDefault));
            h_cap = bytes * 2;
        }
        std::memcpy(h_tables, from, bytes);
        HIP_TRY(d_tables.ensure(bytes));
        HIP_TRY(hipMemcpyAsync(d_tables.p, h_tables, bytes, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipEventRecord(copied, stream));
        pending = true;
        return MR_OK;
    }
    void release()
    {
        d_tables.release();
        if (h_tables) (void)hipHostFree(h_tables);
        if (copied) (void)hipEventDestroy(copied);
        h_tables = nullptr; h_cap = 0; copied = nullptr; pending = false;
    }
};

// ---- the device buffers of a debug entry: released when it returns, by whichever way, once the library's stream has drained
struct Drained {
    std::vector<DevBuf *> bufs;
    Drained(std::initializer_list<DevBuf *> b) : bufs(b) {}
    Drained(const Drained &) = delete;
    ~Drained()
    {
        if (g_initialised) (void)hipStreamSynchronize(g_stream);
        for (DevBuf *d : bufs) d->release();
    }
};

// ---- the checks
// a weight, a scale, a radius as the kernels take it: float32, finite and positive
inline bool positive_f32(double v, float &out)
{
    out = (float)v;
    return std::isfinite(out) && out > 0.0f;
}

// a description's depth map (Z -> eye depth, ao_eye_depth) into the pass's parameters
inline int take_depth_map(const char *pass, const double *depth_map, double *m)
{
    for (int i = 0; i < 4; ++i) {
        if (!std::isfinite(depth_map[i])) return fail(MR_E_INVALID, std::string(pass) + ": the depth map must be finite");
        m[i] = depth_map[i];
    }
    return MR_OK;
}

// a frame, a sample grid or a field of a debug entry: the kernels' coordinates are 16-bit
inline bool frame_size_ok(int32_t height, int32_t width) { return height > 0 && width > 0 && height <= 32767 && width <= 32767; }

// eye depth of a z-buffer value as the mirrors take it; +inf: background
inline float host_eye_depth(const double m[4], double z)
{
    const float v = mr::ao_eye_depth(m, z);
    return std::isfinite(z) && std::isfinite(v) ? v : std::numeric_limits<float>::infinity();
}

}  // namespace
