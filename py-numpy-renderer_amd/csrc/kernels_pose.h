// kernels_pose.h -- the kernels only the pose pass runs (host_pose.h, apply_poses): a model's pose changes vertex
// positions -- and, where the caller asked for it (mr_scene_set_model_pose_normals), the shading normals -- so the records
// that depend on them are rebuilt on the device, in front of the frame.
//
//   k_pose_vertices   vertices of the posed models: pristine vertex @ pose, the ascending fma chain of
//                     mr_host_matmul_chain, bit for bit
//   k_pose_normals    vertex normals of the models that have a normal matrix G: float32(pristine normal @ G), the same chain
//   k_pose_texels     the same for the texels of those models' object-space normal maps, into copies of the maps
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
