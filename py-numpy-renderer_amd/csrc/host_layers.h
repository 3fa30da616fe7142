// host_layers.h -- the per-sample data layers (layers_def.h has the definition): the scene's description and its checks,
// the layer buffers a frame slot owns, the launch of k_layers right behind a frame's k_tile, the same arithmetic on the
// host, bit for bit (host_layers: plain C++, no device), and mr_debug_layers_post, the kernel on arrays a caller supplies.
#pragma once

namespace {

inline int layers_linked()
{
    return linked("this library was linked without layers.hip: no data layers (build it with __graft_entry__.build())", &mr_layers::launch);
}

// a description into the kernel's parameters; n_faces is the caller's
int layers_params(const mr_layers_desc *d, int32_t n_faces, mr::LayersParams &p)
{
    if (!d) return fail(MR_E_INVALID, "data layers: the description is NULL");
    if (d->mask <= 0 || (d->mask & ~mr::LAYER_ALL)) return fail(MR_E_INVALID, "data layers: the mask must name at least one of the layers 0 .. 8 and nothing else");
    if (d->n_models < 1) return fail(MR_E_INVALID, "data layers: at least one model");
    for (int i = 0; i < 16; ++i) {
        if (!std::isfinite(d->s[i])) return fail(MR_E_INVALID, "data layers: an entry of s is not finite");
        p.s[i] = d->s[i];
    }
    p.mask = d->mask; p.n_models = d->n_models; p.n_faces = n_faces; p.pad = 0;
    return MR_OK;
}

// what the mirror and the debug entry refuse of the tables and the winner map
int layers_check_map(const int32_t *winner, const int32_t *face_off, int32_t n_models, int32_t n_faces, int32_t height, int32_t width)
{
    if (n_faces < 0) return fail(MR_E_INVALID, "data layers: a negative count");
    for (int32_t m = 0; m < n_models; ++m)
        if (face_off[m] < 0 || face_off[m] > n_faces || (m > 0 && face_off[m] < face_off[m - 1]) || (m == 0 && face_off[0] != 0))
            return fail(MR_E_INVALID, "data layers: the models' first faces must ascend from 0 to at most the number of faces");
    const size_t n = (size_t)height * width;
    for (size_t i = 0; i < n; ++i)
        if (winner[i] >= n_faces) return fail(MR_E_INVALID, "data layers: a winner is not a face");
    return MR_OK;
}

inline size_t layer_bytes(int layer, size_t n_samples) { return n_samples * (size_t)mr::layer_words(layer) * 4; }

// one sample of the mirror into the caller's arrays
inline void layers_store(void *const *out, int32_t mask, size_t i, int32_t model, int32_t face, int32_t material, const mr::LayerSample &o)
{
    using namespace mr;
    if (mask & (1 << LAYER_MODEL)) static_cast<int32_t *>(out[LAYER_MODEL])[i] = model;
    if (mask & (1 << LAYER_FACE)) static_cast<int32_t *>(out[LAYER_FACE])[i] = face;
    if (mask & (1 << LAYER_MATERIAL)) static_cast<int32_t *>(out[LAYER_MATERIAL])[i] = material;
    if (mask & (1 << LAYER_DEPTH)) static_cast<float *>(out[LAYER_DEPTH])[i] = o.depth;
    const struct { int layer; const float *v; int n; } wide[] = { { LAYER_BARYCENTRIC, o.bary, 3 }, { LAYER_POSITION, o.position, 3 },
                                                                  { LAYER_FACE_NORMAL, o.face_normal, 3 }, { LAYER_NORMAL, o.normal, 3 }, { LAYER_UV, o.uv, 2 } };
    for (const auto &l : wide)
        if (mask & (1 << l.layer))
            for (int j = 0; j < l.n; ++j) static_cast<float *>(out[l.layer])[i * l.n + j] = l.v[j];
}

// k_layers on the host
int host_layers(const int32_t *winner, int32_t height, int32_t width, const void *face_pos, int32_t pos32, const float *face_attr, int32_t n_faces,
                const int32_t *face_off, const mr_layers_desc *d, void *const *out, int64_t *out_degenerate)
{
    using namespace mr;
    if (!winner || !face_pos || !face_attr || !face_off || !d || !out) return fail(MR_E_INVALID, "mr_host_layers: NULL argument");
    if (!frame_size_ok(height, width)) return fail(MR_E_INVALID, "mr_host_layers: resolution out of range");
    LayersParams p;
    if (int rc = layers_params(d, n_faces, p)) return rc;
    for (int l = 0; l < N_LAYERS; ++l)
        if ((p.mask & (1 << l)) && !out[l]) return fail(MR_E_INVALID, "mr_host_layers: a layer the mask names has no array");
    if (int rc = layers_check_map(winner, face_off, p.n_models, n_faces, height, width)) return rc;
    const FaceAttr *attr = reinterpret_cast<const FaceAttr *>(face_attr);
    int64_t degenerate = 0;
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
            const size_t i = (size_t)y * width + x;
            const int32_t w = winner[i];
            int32_t model = -1, face = -1, material = -1;
            LayerSample o;
            layers_background(o);
            if (w >= 0) {
                model = motion_model_of(face_off, p.n_models, w);
                face = w - face_off[model];
                if (pos32) {
                    const FacePos32 &fp = static_cast<const FacePos32 *>(face_pos)[w];
                    material = fp.material;
                    layers_sample(fp, attr[w], p.s, LAYER_ALL, x, y, o);
                } else {
                    const FacePos64 &fp = static_cast<const FacePos64 *>(face_pos)[w];
                    material = fp.material;
                    layers_sample(fp, attr[w], p.s, LAYER_ALL, x, y, o);
                }
                degenerate += o.degenerate ? 1 : 0;
            }
            layers_store(out, p.mask, i, model, face, material, o);
        }
    if (out_degenerate) *out_degenerate = degenerate;
    return MR_OK;
}

// What a frame slot owns for the pass: one buffer a layer, grown on demand.
struct LayersSlot {
    DevBuf d[mr::N_LAYERS];
    void release() { for (DevBuf &b : d) b.release(); }
};

void layers_release(mr_scene *sc)
{
    sc->layers.d_face_off.release();
    release_pass(sc->layers);
}

// k_layers on the frame's stream, behind k_tile, marked for mr_debug_layers_times.  The models' first faces live on the
// device once per commit: commit() has waited for every frame that read the previous table.
int launch_layers(mr_scene *sc, hipStream_t stream, LayersSlot &ls, const int32_t *winner, int width, int height, mr::LayersParams p)
{
    mr_scene::Layers &a = sc->layers;
    const int32_t n_models = (int32_t)sc->model_face_off.size();
    if (a.table_commits != sc->commits) {
        HIP_TRY(a.d_face_off.ensure(std::max<size_t>((size_t)n_models * sizeof(int32_t), 16)));
        if (n_models) HIP_TRY(hipMemcpy(a.d_face_off.p, sc->model_face_off.data(), (size_t)n_models * sizeof(int32_t), hipMemcpyHostToDevice));
        a.table_commits = sc->commits;
    }
    p.n_models = n_models;
    p.n_faces = (int32_t)(sc->faces.size() / 12);
    const size_t n = (size_t)width * height;
    mr::LayersArgs args;
    std::memset(&args, 0, sizeof args);
    args.winner = winner; args.face_pos = sc->d_face_pos.p; args.face_attr = sc->d_face_attr.as<mr::FaceAttr>();
    args.face_off = a.d_face_off.as<int32_t>();
    args.width = width; args.height = height;
    for (int l = 0; l < mr::N_LAYERS; ++l)
        if (p.mask & (1 << l)) {
            HIP_TRY(ls.d[l].ensure(layer_bytes(l, n)));
            args.out[l] = ls.d[l].p;
        }
    const int rc = marked_launch(a, stream, width, height, [&] { mr_layers::launch(stream, args, p, sc->pos32 ? 1 : 0); return MR_OK; });
    if (rc == MR_OK) a.last_mask = p.mask;
    return rc;
}

constexpr size_t LAYERS_GUARD = 256;                     // bytes of sentinel in front of and behind each output buffer
constexpr unsigned char LAYERS_SENTINEL = 0xa5;

// mr_debug_layers_post: the kernel on the caller's arrays through the library's own launch.  Every layer's buffer lies
// between guards of sentinel bytes and starts as sentinel.  Every refusal comes before any device call; the scene lends its
// error text only.
int debug_layers_post(mr_scene *sc, const int32_t *winner, int32_t height, int32_t width, const void *face_pos, int32_t pos32, const float *face_attr,
                      int32_t n_faces, const int32_t *face_off, const mr_layers_desc *d, void *const *out, int32_t *out_guard, float *out_ms)
{
    using namespace mr;
    if (!sc || !winner || !face_pos || !face_attr || !face_off || !d || !out || !out_guard) return fail(MR_E_INVALID, "mr_debug_layers_post: NULL argument");
    for (int l = 0; l < N_LAYERS; ++l)
        if (!out[l]) return fail(MR_E_INVALID, "mr_debug_layers_post: NULL argument");
    if (!frame_size_ok(height, width)) return fail(MR_E_INVALID, "mr_debug_layers_post: resolution out of range");
    LayersParams p;
    if (int rc = layers_params(d, n_faces, p)) return rc;
    if (int rc = layers_check_map(winner, face_off, p.n_models, n_faces, height, width)) return rc;
    if (int rc = layers_linked()) return rc;
    if (int rc = ensure_init()) return rc;
    const size_t n = (size_t)height * width, G = LAYERS_GUARD, pos_bytes = pos32 ? sizeof(FacePos32) : sizeof(FacePos64);
    const std::vector<int32_t> wv(winner, winner + n), ov(face_off, face_off + p.n_models);
    const std::vector<unsigned char> pv(static_cast<const unsigned char *>(face_pos), static_cast<const unsigned char *>(face_pos) + (size_t)n_faces * pos_bytes);
    const std::vector<float> av(face_attr, face_attr + (size_t)n_faces * 16);
    std::vector<unsigned char> guards(2 * G * N_LAYERS);
    struct { DevBuf winner, off, pos, attr, out[N_LAYERS]; } buf;
    Drained drained{ &buf.winner, &buf.off, &buf.pos, &buf.attr, &buf.out[0], &buf.out[1], &buf.out[2], &buf.out[3], &buf.out[4], &buf.out[5],
                     &buf.out[6], &buf.out[7], &buf.out[8] };                       // (behind the vectors: it drains the stream before they go)
    static_assert(N_LAYERS == 9, "one buffer a layer");
    Marks<2> marks;
    struct MarksGuard { Marks<2> &m; ~MarksGuard() { m.release(); } } marks_guard{ marks };
    if (int rc = upload(buf.winner, wv, g_stream)) return rc;
    if (int rc = upload(buf.off, ov, g_stream)) return rc;
    if (int rc = upload(buf.pos, pv, g_stream)) return rc;
    if (int rc = upload(buf.attr, av, g_stream)) return rc;
    LayersArgs args;
    std::memset(&args, 0, sizeof args);
    args.winner = buf.winner.as<int32_t>(); args.face_pos = buf.pos.p; args.face_attr = buf.attr.as<FaceAttr>(); args.face_off = buf.off.as<int32_t>();
    args.width = width; args.height = height;
    for (int l = 0; l < N_LAYERS; ++l) {
        const size_t bytes = layer_bytes(l, n) + 2 * G;
        HIP_TRY(buf.out[l].ensure(bytes));
        HIP_TRY(hipMemsetAsync(buf.out[l].p, LAYERS_SENTINEL, bytes, g_stream));
        args.out[l] = buf.out[l].as<char>() + G;           // (every layer has a buffer here, named or not: the kernel must leave the others alone)
    }
    if (out_ms) { if (int rc = marks.create()) return rc; if (int rc = marks.record(0, g_stream)) return rc; }
    mr_layers::launch(g_stream, args, p, pos32 ? 1 : 0);
    if (out_ms) { if (int rc = marks.record(1, g_stream)) return rc; }
    HIP_TRY(hipGetLastError());
    for (int l = 0; l < N_LAYERS; ++l) {
        const size_t bytes = layer_bytes(l, n);
        HIP_TRY(hipMemcpyAsync(guards.data() + (size_t)l * 2 * G, buf.out[l].p, G, hipMemcpyDeviceToHost, g_stream));
        HIP_TRY(hipMemcpyAsync(guards.data() + (size_t)l * 2 * G + G, buf.out[l].as<char>() + G + bytes, G, hipMemcpyDeviceToHost, g_stream));
        HIP_TRY(hipMemcpyAsync(out[l], buf.out[l].as<char>() + G, bytes, hipMemcpyDeviceToHost, g_stream));
    }
    HIP_TRY(hipStreamSynchronize(g_stream));
    if (out_ms)
        if (int rc = marks.elapsed(0, 1, out_ms)) return rc;
    int32_t touched = 0;
    for (unsigned char g : guards) touched += g != LAYERS_SENTINEL;
    *out_guard = touched;
    return MR_OK;
}

}  // namespace
