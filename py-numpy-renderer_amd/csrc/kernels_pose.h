// kernels_pose.h -- the kernels only the pose pass runs (host_pose.h, apply_poses): a model's pose changes vertex
// positions -- and, where the caller asked for it (mr_scene_set_model_pose_normals), the shading normals -- so the records
// that depend on them are rebuilt on the device, in front of the frame.
//
//   k_pose_vertices   vertices of the posed models: pristine vertex @ pose, the ascending fma chain of
//                     mr_host_matmul_chain, bit for bit
//   k_pose_normals    vertex normals of the models that have a normal matrix G: float32(pristine normal @ G), the same chain
//   k_pose_texels     the same for the texels of those models' object-space normal maps, into copies of the maps
//   k_skin_vertices   vertices of the models that have a skin and bones: pristine vertex @ (the vertex's blend of four
//                     bone matrices), then @ pose where the model has one; mr_host_skin_chain, bit for bit
//   k_skin_normals    vertex normals of the models whose normals follow their skin: the owner's blend matrix, then G
//   k_morph_vertices  vertices of the models that have morph targets and weights: pristine vertex plus the weighted
//                     deltas of the targets that list it, an fma chain in ascending target order over sliced per-vertex
//                     lists (host_morph.h); mr_host_morph_chain, bit for bit.  Runs first: skin and pose take its result
//   k_morph_normals   the same over vertex normals, widened and rounded to float32 once
//   k_auto_normals    vertex normals of the models that asked for them rebuilt from the moved vertices: the sum of the
//                     incident faces' cross products over sliced per-normal face lists (host_autonormals.h), normalised
//                     and rounded to float32 once; mr_host_auto_normals, bit for bit.  Runs after the vertex kernels
//   k_clusters        the per-cluster records (rast_types.h, ClusterRec) from the posed vertices: what build_clusters
//                     (host_scene.h) builds on the host at commit time, one wavefront per cluster
//
// The other static records are rebuilt by the kernels a commit runs (k_face_normals, k_edge_normals, k_face_static).
#pragma once

namespace mr {

// One posed model: its vertex range in the scene's array, its pose (row-major, row vectors) and the first of the
// workgroups of k_pose_vertices that cover the range.
struct alignas(16) PoseRow {
    int32_t first, count;
    int32_t block0, pad;
    double m[16];
};
static_assert(sizeof(PoseRow) == 144, "PoseRow layout");
constexpr int POSE_BLOCK = 256;

// One vertex per thread.  block_row[b] is the PoseRow workgroup b works for (filled in by the host: no thread searches),
// so the matrix is uniform over the workgroup and read with scalar loads.  A lane reads and writes its vertex as one
// 32-byte access, consecutive lanes consecutive vertices.
__global__ void __launch_bounds__(POSE_BLOCK)
k_pose_vertices(const PoseRow *__restrict__ rows, const int32_t *__restrict__ block_row, const double4 *__restrict__ verts0,
                double4 *__restrict__ verts)
{
    const PoseRow &r = rows[block_row[blockIdx.x]];
    const int i = (int)(blockIdx.x - (uint32_t)r.block0) * POSE_BLOCK + (int)threadIdx.x;
    if (i >= r.count) return;
    const double4 v = verts0[(size_t)r.first + i];
    double4 o;
    o.x = chain4(v.x, v.y, v.z, v.w, r.m[0], r.m[4], r.m[8], r.m[12]);
    o.y = chain4(v.x, v.y, v.z, v.w, r.m[1], r.m[5], r.m[9], r.m[13]);
    o.z = chain4(v.x, v.y, v.z, v.w, r.m[2], r.m[6], r.m[10], r.m[14]);
    o.w = chain4(v.x, v.y, v.z, v.w, r.m[3], r.m[7], r.m[11], r.m[15]);
    verts[(size_t)r.first + i] = o;
}

// One model's vertex normals (k_pose_normals: first / count index the scene's normal array) or one object-space normal
// map of one model (k_pose_texels: src / dst are the map and its re-baked copy, count its texels), the 3 x 3 matrix G
// (row-major, row vectors) and the first of the workgroups that cover the range.
struct alignas(8) Vec3Row {
    const float *src;
    float *dst;
    int64_t count;
    int32_t first, block0;
    double g[9];
};
static_assert(sizeof(Vec3Row) == 104, "Vec3Row layout");

// float32(v @ G) of one float32 3-vector: widened, every component rn(v0 * G0j) followed by fma steps in ascending k,
// rounded to float32 once (_pack.posed_normals, bit for bit: the library is built with -ffp-contract=off).  A lane
// reads and writes its 12 bytes, consecutive lanes consecutive vectors; G is uniform over the workgroup.
__device__ __forceinline__ void pose_vec3(const Vec3Row &r, const float *__restrict__ src, float *__restrict__ dst, int64_t i)
{
    const float3 v = *reinterpret_cast<const float3 *>(src + i * 3);
    const double x = (double)v.x, y = (double)v.y, z = (double)v.z;
    float3 o;
    o.x = (float)chain3(x, y, z, r.g[0], r.g[3], r.g[6]);
    o.y = (float)chain3(x, y, z, r.g[1], r.g[4], r.g[7]);
    o.z = (float)chain3(x, y, z, r.g[2], r.g[5], r.g[8]);
    *reinterpret_cast<float3 *>(dst + i * 3) = o;
}

// One normal per thread, the scheme of k_pose_vertices: block_row[b] is the row workgroup b works for.
__global__ void __launch_bounds__(POSE_BLOCK)
k_pose_normals(const Vec3Row *__restrict__ rows, const int32_t *__restrict__ block_row, const float *__restrict__ normals0,
               float *__restrict__ normals)
{
    const Vec3Row &r = rows[block_row[blockIdx.x]];
    const int64_t i = (int64_t)(blockIdx.x - (uint32_t)r.block0) * POSE_BLOCK + (int64_t)threadIdx.x;
    if (i >= r.count) return;
    pose_vec3(r, normals0 + (size_t)r.first * 3, normals + (size_t)r.first * 3, i);
}

// One texel per thread of every (model with G, object-space normal map) pair, the same two tables.
__global__ void __launch_bounds__(POSE_BLOCK)
k_pose_texels(const Vec3Row *__restrict__ rows, const int32_t *__restrict__ block_row)
{
    const Vec3Row &r = rows[block_row[blockIdx.x]];
    const int64_t i = (int64_t)(blockIdx.x - (uint32_t)r.block0) * POSE_BLOCK + (int64_t)threadIdx.x;
    if (i >= r.count) return;
    pose_vec3(r, r.src, r.dst, i);
}

// One skinned model (mr_scene_set_model_skin / mr_scene_set_model_bones): its vertex range, where its joints and
// weights start in the scene's skin tables, where its bones start in the pass's bone table, the pose that follows the
// skin (if the model has one) and the first of the workgroups of k_skin_vertices that cover the range.
struct alignas(16) SkinRow {
    int32_t first, count;
    int32_t block0, table_off;
    int32_t bone0, n_bones, has_pose, pad;
    double m[16];
};
static_assert(sizeof(SkinRow) == 160, "SkinRow layout");

// Row r of the blend matrix S of one vertex: S[r][c] = rn(w0 * B[j0][r][c]) followed by fma steps over slots 1..3
// (_fp.dot_chain over the four slots).  A bone is 16 doubles, row-major: row r is one 32-byte load per slot, from a
// table of a few kilobytes that every lane of the pass reads (the gathers differ per lane; the table stays in cache).
__device__ __forceinline__ double4 skin_row(const double4 *__restrict__ bones, const int4 j, const double4 w, int r)
{
    const double4 b0 = bones[(size_t)j.x * 4 + r], b1 = bones[(size_t)j.y * 4 + r];
    const double4 b2 = bones[(size_t)j.z * 4 + r], b3 = bones[(size_t)j.w * 4 + r];
    double4 s;
    s.x = chain4(w.x, w.y, w.z, w.w, b0.x, b1.x, b2.x, b3.x);
    s.y = chain4(w.x, w.y, w.z, w.w, b0.y, b1.y, b2.y, b3.y);
    s.z = chain4(w.x, w.y, w.z, w.w, b0.z, b1.z, b2.z, b3.z);
    s.w = chain4(w.x, w.y, w.z, w.w, b0.w, b1.w, b2.w, b3.w);
    return s;
}

// One vertex per thread of the skinned models, the tables of k_pose_vertices.  v @ S is the ascending chain over the
// rows of S, so S is formed and used row by row: rn(v0 * S[0][c]), then one fma per further row (mr_host_skin_chain,
// bit for bit).  The row's pose, if any, follows as in k_pose_vertices.  One 32-byte load and one 32-byte store per lane.
// STAGED: the workgroup first copies its model's bones into LDS and the lanes gather from there (measured a little
// faster than gathering from the cached table: DESIGN.md section 6e); the host launches it only when every skinned
// model of the pass has at most SKIN_LDS_BONES bones, and the plain kernel otherwise.
constexpr int SKIN_LDS_BONES = 64;                                 // 8 KB of LDS per workgroup

template <bool STAGED>
__global__ void __launch_bounds__(POSE_BLOCK)
k_skin_vertices(const SkinRow *__restrict__ rows, const int32_t *__restrict__ block_row, const double4 *__restrict__ verts0,
                const int4 *__restrict__ joints, const double4 *__restrict__ weights, const double4 *__restrict__ bones,
                double4 *__restrict__ verts)
{
    const SkinRow &r = rows[block_row[blockIdx.x]];
    const int i = (int)(blockIdx.x - (uint32_t)r.block0) * POSE_BLOCK + (int)threadIdx.x;
    __shared__ double4 staged[STAGED ? SKIN_LDS_BONES * 4 : 1];
    if constexpr (STAGED) {                                        // (before any lane leaves: every lane meets the barrier)
        for (int k = (int)threadIdx.x; k < min(r.n_bones, SKIN_LDS_BONES) * 4; k += POSE_BLOCK) staged[k] = bones[(size_t)r.bone0 * 4 + k];
        __syncthreads();
    }
    if (i >= r.count) return;
    const double4 v = verts0[(size_t)r.first + i];
    const int4 j = joints[(size_t)r.table_off + i];
    const double4 w = weights[(size_t)r.table_off + i];
    const double4 *b = STAGED ? staged : bones + (size_t)r.bone0 * 4;
    double4 s = skin_row(b, j, w, 0);
    double4 o;
    o.x = v.x * s.x; o.y = v.x * s.y; o.z = v.x * s.z; o.w = v.x * s.w;
    s = skin_row(b, j, w, 1);
    o.x = fma(v.y, s.x, o.x); o.y = fma(v.y, s.y, o.y); o.z = fma(v.y, s.z, o.z); o.w = fma(v.y, s.w, o.w);
    s = skin_row(b, j, w, 2);
    o.x = fma(v.z, s.x, o.x); o.y = fma(v.z, s.y, o.y); o.z = fma(v.z, s.z, o.z); o.w = fma(v.z, s.w, o.w);
    s = skin_row(b, j, w, 3);
    o.x = fma(v.w, s.x, o.x); o.y = fma(v.w, s.y, o.y); o.z = fma(v.w, s.z, o.z); o.w = fma(v.w, s.w, o.w);
    if (r.has_pose) {                                              // (uniform over the workgroup)
        const double4 p = o;
        o.x = chain4(p.x, p.y, p.z, p.w, r.m[0], r.m[4], r.m[8], r.m[12]);
        o.y = chain4(p.x, p.y, p.z, p.w, r.m[1], r.m[5], r.m[9], r.m[13]);
        o.z = chain4(p.x, p.y, p.z, p.w, r.m[2], r.m[6], r.m[10], r.m[14]);
        o.w = chain4(p.x, p.y, p.z, p.w, r.m[3], r.m[7], r.m[11], r.m[15]);
    }
    verts[(size_t)r.first + i] = o;
}

// One model whose vertex normals follow its skin: its normal range, where its owner table (per normal: the vertex of
// the model whose blend matrix the normal takes, -1: the normal stays) and its joints and weights start, its bones, the
// normal matrix G that follows the skin (if the model has one) and the first of its workgroups.
struct alignas(8) SkinNormalRow {
    int32_t first, count;
    int32_t block0, owner_off;
    int32_t table_off, bone0, has_g, pad;
    double g[9];
};
static_assert(sizeof(SkinNormalRow) == 104, "SkinNormalRow layout");

// One normal per thread: n' = float64(float32 normal) @ S[:3, :3] of the owner (rows 0..2 of S, the chain of
// k_skin_vertices without its last step), then n' @ G where the row has one, then ONE rounding to float32.
__global__ void __launch_bounds__(POSE_BLOCK)
k_skin_normals(const SkinNormalRow *__restrict__ rows, const int32_t *__restrict__ block_row, const float *__restrict__ normals0,
               const int32_t *__restrict__ owners, const int4 *__restrict__ joints, const double4 *__restrict__ weights,
               const double4 *__restrict__ bones, float *__restrict__ normals)
{
    const SkinNormalRow &r = rows[block_row[blockIdx.x]];
    const int i = (int)(blockIdx.x - (uint32_t)r.block0) * POSE_BLOCK + (int)threadIdx.x;
    if (i >= r.count) return;
    const size_t at = ((size_t)r.first + i) * 3;
    const float3 n = *reinterpret_cast<const float3 *>(normals0 + at);
    double x = (double)n.x, y = (double)n.y, z = (double)n.z;
    const int owner = owners[(size_t)r.owner_off + i];
    if (owner >= 0) {
        const int4 j = joints[(size_t)r.table_off + owner];
        const double4 w = weights[(size_t)r.table_off + owner];
        const double4 *b = bones + (size_t)r.bone0 * 4;
        double4 s = skin_row(b, j, w, 0);
        double ox = x * s.x, oy = x * s.y, oz = x * s.z;
        s = skin_row(b, j, w, 1);
        ox = fma(y, s.x, ox); oy = fma(y, s.y, oy); oz = fma(y, s.z, oz);
        s = skin_row(b, j, w, 2);
        ox = fma(z, s.x, ox); oy = fma(z, s.y, oy); oz = fma(z, s.z, oz);
        x = ox; y = oy; z = oz;
    }
    float3 o;
    if (r.has_g) {
        o.x = (float)chain3(x, y, z, r.g[0], r.g[3], r.g[6]);
        o.y = (float)chain3(x, y, z, r.g[1], r.g[4], r.g[7]);
        o.z = (float)chain3(x, y, z, r.g[2], r.g[5], r.g[8]);
    } else {
        o.x = (float)x; o.y = (float)y; o.z = (float)z;
    }
    *reinterpret_cast<float3 *>(normals + at) = o;
}

// One morphed model (mr_scene_set_model_morph / mr_scene_set_model_morph_weights): its vertex (k_morph_vertices) or
// normal (k_morph_normals) range, where its slices start in the slice table, where its weights start in the pass's
// weight table, and the first of the workgroups that cover the range.  direct: nothing follows the morph (no skin, no
// pose / no normal matrix), so the result goes straight into the array every frame kernel reads; otherwise into the
// array the skin and pose kernels take as their pristine source.
struct alignas(8) MorphRow {
    int32_t first, count;
    int32_t block0, slice0;
    int32_t weight0, n_targets, direct, pad;
};
static_assert(sizeof(MorphRow) == 32, "MorphRow layout");
static_assert(POSE_BLOCK % WAVE == 0, "a wavefront of the morph kernels walks one slice");

// The morph kernels' body: one vertex (float64 x y z w, w passes through) or one normal (float32 x y z, widened, rounded
// once at the end) per thread, the tables of k_pose_vertices.  A wavefront holds 64 consecutive vertices of the model:
// one slice of its contribution lists (host_morph.h).  Entry e of lane l sits at slice_first[s] + e * 64 + l in the
// four planes, so every load of the walk is one contiguous 256-byte (target) or 512-byte (delta component) access and
// the trip count is uniform over the wavefront; padding (target -1) is skipped.  Every listed target takes its fma step,
// in ascending target order (mr_host_morph_chain, bit for bit), also with a weight of 0.  The one gather is w[target],
// from a table of 8 bytes per target that every workgroup of the model reads: it stays in cache (staging it in LDS was
// built and timed too and was no faster: DESIGN.md section 6f).
template <bool NORMALS>
__device__ __forceinline__ void morph_body(const MorphRow *__restrict__ rows, const int32_t *__restrict__ block_row,
                                           const int32_t *__restrict__ slice_first, const int32_t *__restrict__ target,
                                           const double *__restrict__ dx, const double *__restrict__ dy, const double *__restrict__ dz,
                                           const double *__restrict__ weights, const void *__restrict__ src, void *__restrict__ held,
                                           void *__restrict__ live)
{
    const MorphRow &r = rows[block_row[blockIdx.x]];
    const int i = (int)(blockIdx.x - (uint32_t)r.block0) * POSE_BLOCK + (int)threadIdx.x;
    if (i >= r.count) return;
    const double *w = weights + (size_t)r.weight0;
    const size_t at = (size_t)r.first + i;
    double x, y, z, h = 0.0;
    if constexpr (NORMALS) {
        const float3 n = *reinterpret_cast<const float3 *>(static_cast<const float *>(src) + at * 3);
        x = (double)n.x; y = (double)n.y; z = (double)n.z;
    } else {
        const double4 v = static_cast<const double4 *>(src)[at];
        x = v.x; y = v.y; z = v.z; h = v.w;
    }
    const int s = __builtin_amdgcn_readfirstlane(r.slice0 + (i >> 6)), lane = i & (WAVE - 1);     // (i >> 6 is the wavefront's)
    const int end = slice_first[s + 1];
    for (int p = slice_first[s]; p < end; p += WAVE) {
        const int t = target[(size_t)p + lane];
        if (t < 0) continue;
        const double wt = w[t];
        x = fma(wt, dx[(size_t)p + lane], x);
        y = fma(wt, dy[(size_t)p + lane], y);
        z = fma(wt, dz[(size_t)p + lane], z);
    }
    void *dst = r.direct ? live : held;                            // (uniform over the workgroup)
    if constexpr (NORMALS) {
        float3 o;
        o.x = (float)x; o.y = (float)y; o.z = (float)z;
        *reinterpret_cast<float3 *>(static_cast<float *>(dst) + at * 3) = o;
    } else {
        double4 o;
        o.x = x; o.y = y; o.z = z; o.w = h;
        static_cast<double4 *>(dst)[at] = o;
    }
}

__global__ void __launch_bounds__(POSE_BLOCK)
k_morph_vertices(const MorphRow *__restrict__ rows, const int32_t *__restrict__ block_row, const int32_t *__restrict__ slice_first,
                 const int32_t *__restrict__ target, const double *__restrict__ dx, const double *__restrict__ dy,
                 const double *__restrict__ dz, const double *__restrict__ weights, const double4 *__restrict__ verts0,
                 double4 *__restrict__ verts_m, double4 *__restrict__ verts)
{
    morph_body<false>(rows, block_row, slice_first, target, dx, dy, dz, weights, verts0, verts_m, verts);
}

__global__ void __launch_bounds__(POSE_BLOCK)
k_morph_normals(const MorphRow *__restrict__ rows, const int32_t *__restrict__ block_row, const int32_t *__restrict__ slice_first,
                const int32_t *__restrict__ target, const double *__restrict__ dx, const double *__restrict__ dy,
                const double *__restrict__ dz, const double *__restrict__ weights, const float *__restrict__ normals0,
                float *__restrict__ normals_m, float *__restrict__ normals)
{
    morph_body<true>(rows, block_row, slice_first, target, dx, dy, dz, weights, normals0, normals_m, normals);
}

// One model whose vertex normals are rebuilt from its deformed mesh (mr_scene_set_model_auto_normals): its normal range,
// where its slices start in the slice table of the face lists, and the first of the workgroups that cover the range.
struct alignas(8) AutoRow {
    int32_t first, count;
    int32_t block0, slice0;
};
static_assert(sizeof(AutoRow) == 16, "AutoRow layout");

// One normal per thread, the tables of k_morph_normals: a wavefront holds 64 consecutive normals of the model, one
// slice of its face lists (host_autonormals.h).  Entry e of lane l sits at slice_first[s] + e * 64 + l, so the list is
// read as contiguous 256-byte accesses and the trip count is uniform over the wavefront; padding (-1) is skipped.  Per
// entry: the face, its three vertex columns from the face table, three gathered 32-byte vertices, the cross product
// of the double branch of face_unit_normal and three adds -- the first product is taken as it is, so that a -0 stays
// one -- in ascending face order (mr_host_auto_normals, bit for bit: the library is built with -ffp-contract=off).
// After the walk normalize3's arithmetic, rounded to float32 once; the authored normal (normals0) stays for an empty
// list, a sum of length 0 and a sum or length that is not finite.  kept[w] counts those of wavefront w of the launch
// (written by one lane; read by mr_debug_auto_normals).  The indices were validated when the model was added.  (Lists
// that hold the three vertex columns themselves, 12 bytes an entry, were built and timed too: DESIGN.md section 6g.)
__global__ void __launch_bounds__(POSE_BLOCK)
k_auto_normals(const AutoRow *__restrict__ rows, const int32_t *__restrict__ block_row, const int32_t *__restrict__ slice_first,
               const int32_t *__restrict__ face_list, const int32_t *__restrict__ faces, const double4 *__restrict__ verts,
               const float *__restrict__ normals0, float *__restrict__ normals, int32_t *__restrict__ kept)
{
    const AutoRow &r = rows[block_row[blockIdx.x]];
    const int i = (int)(blockIdx.x - (uint32_t)r.block0) * POSE_BLOCK + (int)threadIdx.x;
    if (i >= r.count) return;
    const size_t at = ((size_t)r.first + i) * 3;
    const int s = __builtin_amdgcn_readfirstlane(r.slice0 + (i >> 6)), lane = i & (WAVE - 1);     // (i >> 6 is the wavefront's)
    const int end = slice_first[s + 1];
    double ax = 0.0, ay = 0.0, az = 0.0;
    bool any = false;
    for (int p = slice_first[s]; p < end; p += WAVE) {
        const int f = face_list[(size_t)p + lane];
        if (f < 0) continue;
        const int32_t *fc = faces + (size_t)f * 12;
        const double4 a = verts[fc[0]], b = verts[fc[4]], c = verts[fc[8]];
        const double e0x = b.x - a.x, e0y = b.y - a.y, e0z = b.z - a.z;
        const double e1x = c.x - a.x, e1y = c.y - a.y, e1z = c.z - a.z;
        const double cx = e0y * e1z - e0z * e1y, cy = e0z * e1x - e0x * e1z, cz = e0x * e1y - e0y * e1x;
        ax = any ? ax + cx : cx;
        ay = any ? ay + cy : cy;
        az = any ? az + cz : cz;
        any = true;
    }
    const double l = sqrt((ax * ax + ay * ay) + az * az);
    const bool keep = !any || l == 0 || !isfinite(ax) || !isfinite(ay) || !isfinite(az) || !isfinite(l);
    float3 o;
    if (keep) o = *reinterpret_cast<const float3 *>(normals0 + at);
    else { o.x = (float)(ax / l); o.y = (float)(ay / l); o.z = (float)(az / l); }
    *reinterpret_cast<float3 *>(normals + at) = o;
    const int n_kept = __popcll(__ballot(keep));                    // (of the lanes that have a normal)
    if (lane == 0) kept[blockIdx.x * (POSE_BLOCK / WAVE) + threadIdx.x / WAVE] = n_kept;
}

__device__ __forceinline__ double shfl_xor_d(double v, int mask)
{
    return __hiloint2double(__shfl_xor(__double2hiint(v), mask), __shfl_xor(__double2loint(v), mask));
}
// the float32 at or below / at or above x
__device__ __forceinline__ float f32_down(double x) { const float f = (float)x; return (double)f > x ? nextafterf(f, -INFINITY) : f; }
__device__ __forceinline__ float f32_up(double x) { const float f = (float)x; return (double)f < x ? nextafterf(f, INFINITY) : f; }

// One wavefront per cluster of CLUSTER_FACES faces, one face per lane; minima, maxima and sums go round the wavefront
// by butterfly (every lane ends with the same value: the steps are commutative), lane 0 stores the record.  The guards
// and slacks are build_clusters' own; the normals are summed in another order than its face-by-face loop, so a record
// may differ from the host's in the last bits of the axis -- it is conservative all the same: the box holds every
// corner, and cos_half lies 2e-6 below the least n . axis taken with THIS axis.
__global__ void __launch_bounds__(256)
k_clusters(int n_faces, const int32_t *__restrict__ faces, const double *__restrict__ verts, ClusterRec *__restrict__ out)
{
    static_assert(CLUSTER_FACES == WAVE, "one face per lane");
    const int lane = (int)threadIdx.x & (WAVE - 1);
    const int cid = (int)(blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE);
    const int f0 = cid * CLUSTER_FACES;
    if (f0 >= n_faces) return;                                     // (the whole wavefront)
    const int f = f0 + lane;
    const bool have = f < n_faces;
    const int in_cluster = min(n_faces - f0, CLUSTER_FACES);
    double lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    double n[3] = { 0, 0, 0 };
    bool boxed = true, coned = true;
    if (have) {
        double v[3][4];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double *p = verts + (size_t)faces[(size_t)f * 12 + k * 4] * 4;
#pragma unroll
            for (int j = 0; j < 4; ++j) v[k][j] = p[j];
            if (!(v[k][3] == 1.0)) boxed = false;                  // (a homogeneous coordinate other than 1: no box)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                lo[j] = v[k][j] < lo[j] ? v[k][j] : lo[j];
                hi[j] = v[k][j] > hi[j] ? v[k][j] : hi[j];
                if (!isfinite(v[k][j])) boxed = false;
            }
        }
        const double a[3] = { v[1][0] - v[0][0], v[1][1] - v[0][1], v[1][2] - v[0][2] };
        const double b[3] = { v[2][0] - v[0][0], v[2][1] - v[0][1], v[2][2] - v[0][2] };
        const double c[3] = { a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0] };
        const double l = sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
        if (!(l > 0) || !isfinite(l)) coned = false;               // a face without area: no cone
        else { n[0] = c[0] / l; n[1] = c[1] / l; n[2] = c[2] / l; }
    }
    boxed = __all(boxed);
    coned = __all(coned);
    double sum[3] = { n[0], n[1], n[2] };
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double l = shfl_xor_d(lo[j], off), h = shfl_xor_d(hi[j], off);
            lo[j] = l < lo[j] ? l : lo[j];
            hi[j] = h > hi[j] ? h : hi[j];
            sum[j] += shfl_xor_d(sum[j], off);
        }
    }
    ClusterRec r;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        r.lo[j] = boxed ? f32_down(lo[j]) : NAN;                   // NaN: never culled, every comparison fails
        r.hi[j] = boxed ? f32_up(hi[j]) : NAN;
        r.axis[j] = 0.f;
    }
    r.cos_half = -2.f; r.sin_half = 1.f;
#pragma unroll
    for (int j = 0; j < 5; ++j) r.pad[j] = 0;
    const double sl = sqrt(sum[0] * sum[0] + sum[1] * sum[1] + sum[2] * sum[2]);
    if (coned && sl > 1e-6 * (double)in_cluster) {                 // (wavefront-uniform: every lane holds the same sum)
        double least = have ? (n[0] * sum[0] + n[1] * sum[1] + n[2] * sum[2]) / sl : 1.0;
        least = least < 1.0 ? least : 1.0;
#pragma unroll
        for (int off = 1; off < WAVE; off <<= 1) {
            const double o = shfl_xor_d(least, off);
            least = o < least ? o : least;
        }
        least -= 1e-6;
        if (least > 0.05) {                                        // a cone wider than ~87 degrees never culls anything
#pragma unroll
            for (int j = 0; j < 3; ++j) r.axis[j] = (float)(sum[j] / sl);
            // the axis as stored (float32) is not the axis the dots were taken with: 1e-6 covers it
            r.cos_half = (float)(least - 1e-6);
            const double s = sqrt(fmax(0.0, 1.0 - (double)r.cos_half * (double)r.cos_half)) + 1e-6;
            r.sin_half = (float)(s < 1.0 ? s : 1.0);
        }
    }
    if (lane == 0) out[cid] = r;
}

}  // namespace mr
