// The pose metrics of the 3D validation_step / test_step for a whole Batch (puzzle_diff/model/utils_3d.py:362-383 trans_metrics,
// :415-450 rot_metrics, :916-945 geodesic_distance, :1089-1129 calc_part_acc, as called per object at
// spatial_diffusion_3d_test_double_diffusion.py:895-960, 1036-1080).  DESIGN.md 3k.
//
// k_metrics3d_part: one workgroup per part.  Thread 0 evaluates the three pose metrics of the part's 7-vector pair; all 256
// threads run the K = 1 search both ways between the fragment posed with the prediction (a) and with the target (b).  Both
// posed copies are staged in LDS as component arrays (x[1024] y[1024] z[1024] each, 24 KB together) and never reach memory.
// k_metrics3d_object: one wave per object, the parts of ptr[g] .. ptr[g + 1] summed in index order.
//
// Every expression follows diffassemble_amd/metrics3d.py operation by operation, with contraction off (the host functions
// run mul / add, not fma), so the fp32 rounding is the host route's up to the libm calls; the squared distances alone use an
// fma chain on exact differences.
#include <float.h>
#include <math.h>

#include "da_internal.h"

namespace da {
namespace {

constexpr int M3_THREADS = 256;
constexpr int M3_Q = 4;                          // queries per thread and cloud: one 16-byte LDS read serves 4 x 4 pairs
constexpr int M3_TILE = M3_THREADS * M3_Q;       // points per staged tile, also the queries a workgroup holds at a time
constexpr float M3_FAR = 1e18f;                  // tail of the last candidate group: never the nearest, its square stays finite

struct Pose { float w, x, y, z, tx, ty, tz; };

__device__ __forceinline__ Pose load_pose(const float *__restrict__ r) { return Pose{r[0], r[1], r[2], r[3], r[4], r[5], r[6]}; }

// metrics3d._rotate (t = 2 u x v; v + w t + u x t) + translation.  Staging and queries call this one function with
// contraction off: the same point under the same pose has the same bits wherever it is evaluated (identical poses -> 0).
__device__ __forceinline__ void pose_point(const Pose &q, const float *__restrict__ v, float &X, float &Y, float &Z) {
#pragma clang fp contract(off)
    const float vx = v[0], vy = v[1], vz = v[2];
    const float tx = 2.f * (q.y * vz - q.z * vy), ty = 2.f * (q.z * vx - q.x * vz), tz = 2.f * (q.x * vy - q.y * vx);
    X = ((vx + q.w * tx) + (q.y * tz - q.z * ty)) + q.tx;
    Y = ((vy + q.w * ty) + (q.z * tx - q.x * tz)) + q.ty;
    Z = ((vz + q.w * tz) + (q.x * ty - q.y * tx)) + q.tz;
}

__device__ __forceinline__ float clampf(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }      // NaN passes, as torch.clamp

// metrics3d._euler_zyx_deg: no normalisation of the quaternion
__device__ __forceinline__ void euler_zyx_deg(const Pose &q, float *e) {
#pragma clang fp contract(off)
    const float k = (float)(180.0 / 3.14159265358979323846);
    e[0] = atan2f(2.f * (q.w * q.x + q.y * q.z), 1.f - 2.f * (q.x * q.x + q.y * q.y)) * k;
    e[1] = asinf(clampf(2.f * (q.w * q.y - q.x * q.z), -1.f, 1.f)) * k;
    e[2] = atan2f(2.f * (q.w * q.z + q.x * q.y), 1.f - 2.f * (q.y * q.y + q.z * q.z)) * k;
}

// metrics3d._rmat: scale 2 / |q|^2
__device__ __forceinline__ void rmat(const Pose &q, float *R) {
#pragma clang fp contract(off)
    const float r = q.w, i = q.x, j = q.y, k = q.z;
    const float s = 2.f / (((r * r + i * i) + j * j) + k * k);
    R[0] = 1.f - s * (j * j + k * k); R[1] = s * (i * j - k * r); R[2] = s * (i * k + j * r);
    R[3] = s * (i * j + k * r); R[4] = 1.f - s * (i * i + k * k); R[5] = s * (j * k - i * r);
    R[6] = s * (i * k - j * r); R[7] = s * (j * k + i * r); R[8] = 1.f - s * (i * i + j * j);
}

// (rmse_t, rmse_r, gd_r) of one pose pair
__device__ __forceinline__ void pose_metrics(const Pose &a, const Pose &b, float *o) {
#pragma clang fp contract(off)
    const float dx = a.tx - b.tx, dy = a.ty - b.ty, dz = a.tz - b.tz;
    o[0] = sqrtf(((dx * dx + dy * dy) + dz * dz) / 3.f);
    float e1[3], e2[3], s = 0.f;
    euler_zyx_deg(a, e1);
    euler_zyx_deg(b, e2);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float d = fabsf(e1[c] - e2[c]);
        const float w = 360.f - d;
        d = w < d ? w : d;                                           // torch.minimum: NaN passes
        s += d * d;
    }
    o[1] = sqrtf(s / 3.f);
    float R1[9], R2[9], tr = 0.f;
    rmat(a, R1);
    rmat(b, R2);
#pragma unroll
    for (int c = 0; c < 9; ++c) tr += R1[c] * R2[c];
    // the bounds are torch's: the Python doubles -1 + 1e-6, 1 - 1e-6 rounded to fp32
    o[2] = acosf(clampf(0.5f * (tr - 1.f), (float)(-1.0 + 1e-6), (float)(1.0 - 1e-6)));
}

__device__ __forceinline__ float dist_sq(float ax, float ay, float az, float bx, float by, float bz) {
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    return fmaf(dz, dz, fmaf(dy, dy, dx * dx));
}
__device__ __forceinline__ float min4(float best, float d0, float d1, float d2, float d3) {
    return fminf(fminf(fminf(best, d0), d1), fminf(d2, d3));
}

__global__ __launch_bounds__(M3_THREADS) void k_metrics3d_part(const float *__restrict__ pred, int ld_pred,
                                                                const float *__restrict__ gt, int ld_gt,
                                                                const float *__restrict__ pcds, int N,
                                                                float *__restrict__ per_part) {
    __shared__ float4 tile[2][3][M3_TILE / 4];             // [a | b][x | y | z][group of four points]
    __shared__ float red[2][M3_THREADS / 64];
    const int p = blockIdx.x, tid = threadIdx.x;
    const Pose q1 = load_pose(pred + (size_t)p * ld_pred), q2 = load_pose(gt + (size_t)p * ld_gt);
    float *out = per_part + (size_t)p * 4;
    if (!pcds) {
        if (tid == 0) {
            float o[3];
            pose_metrics(q1, q2, o);
            out[0] = o[0]; out[1] = o[1]; out[2] = o[2]; out[3] = NAN;
        }
        return;
    }
    const float *pts = pcds + (size_t)p * N * 3;
    float *tf = reinterpret_cast<float *>(tile);
    float sum_a = 0.f, sum_b = 0.f;
    for (int q0 = 0; q0 < N; q0 += M3_TILE) {              // this thread's points q0 + tid, + 256, ... of both copies
        float ax[M3_Q], ay[M3_Q], az[M3_Q], bx[M3_Q], by[M3_Q], bz[M3_Q], best_a[M3_Q], best_b[M3_Q];
#pragma unroll
        for (int k = 0; k < M3_Q; ++k) {
            const float *v = pts + (size_t)min(q0 + k * M3_THREADS + tid, N - 1) * 3;
            pose_point(q1, v, ax[k], ay[k], az[k]);
            pose_point(q2, v, bx[k], by[k], bz[k]);
            best_a[k] = FLT_MAX;
            best_b[k] = FLT_MAX;
            // torch.min passes NaN, fminf drops it: a NaN point of either copy makes both means NaN, as on the host
            if (ax[k] != ax[k] || ay[k] != ay[k] || az[k] != az[k] || bx[k] != bx[k] || by[k] != by[k] || bz[k] != bz[k]) sum_a = NAN;
        }
        for (int c0 = 0; c0 < N; c0 += M3_TILE) {          // candidates c0 .. c0 + 1023 of both copies, posed while staged
            __syncthreads();
#pragma unroll
            for (int k = 0; k < M3_Q; ++k) {
                const int ct = k * M3_THREADS + tid, c = c0 + ct;
                float X1 = M3_FAR, Y1 = M3_FAR, Z1 = M3_FAR, X2 = M3_FAR, Y2 = M3_FAR, Z2 = M3_FAR;
                if (c < N) {
                    const float *v = pts + (size_t)c * 3;
                    pose_point(q1, v, X1, Y1, Z1);
                    pose_point(q2, v, X2, Y2, Z2);
                }
                tf[ct] = X1; tf[M3_TILE + ct] = Y1; tf[2 * M3_TILE + ct] = Z1;
                tf[3 * M3_TILE + ct] = X2; tf[4 * M3_TILE + ct] = Y2; tf[5 * M3_TILE + ct] = Z2;
            }
            __syncthreads();
            const int ng = (min(M3_TILE, N - c0) + 3) >> 2;
#pragma unroll 2
            for (int g = 0; g < ng; ++g) {                 // wave-uniform addresses: six 16-byte broadcast reads per 32 pairs
                const float4 cx = tile[1][0][g], cy = tile[1][1][g], cz = tile[1][2][g];
#pragma unroll
                for (int k = 0; k < M3_Q; ++k)             // a_i against four points of b
                    best_a[k] = min4(best_a[k], dist_sq(ax[k], ay[k], az[k], cx.x, cy.x, cz.x), dist_sq(ax[k], ay[k], az[k], cx.y, cy.y, cz.y),
                                     dist_sq(ax[k], ay[k], az[k], cx.z, cy.z, cz.z), dist_sq(ax[k], ay[k], az[k], cx.w, cy.w, cz.w));
                const float4 dx = tile[0][0][g], dy = tile[0][1][g], dz = tile[0][2][g];
#pragma unroll
                for (int k = 0; k < M3_Q; ++k)             // b_j against four points of a
                    best_b[k] = min4(best_b[k], dist_sq(bx[k], by[k], bz[k], dx.x, dy.x, dz.x), dist_sq(bx[k], by[k], bz[k], dx.y, dy.y, dz.y),
                                     dist_sq(bx[k], by[k], bz[k], dx.z, dy.z, dz.z), dist_sq(bx[k], by[k], bz[k], dx.w, dy.w, dz.w));
            }
        }
#pragma unroll
        for (int k = 0; k < M3_Q; ++k)
            if (q0 + k * M3_THREADS + tid < N) { sum_a += best_a[k]; sum_b += best_b[k]; }
    }
    // fixed order, no atomics: lanes by shuffles, then the four waves in order
    for (int o = 32; o > 0; o >>= 1) { sum_a += __shfl_down(sum_a, o, 64); sum_b += __shfl_down(sum_b, o, 64); }
    if ((tid & 63) == 0) { red[0][tid >> 6] = sum_a; red[1][tid >> 6] = sum_b; }
    __syncthreads();
    if (tid == 0) {
        float o[3];
        pose_metrics(q1, q2, o);
        const float sa = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]), sb = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
        out[0] = o[0]; out[1] = o[1]; out[2] = o[2];
        out[3] = sa / (float)N + sb / (float)N;            // d.min(2).mean(1) + d.min(1).mean(1)
    }
}

// One wave per object; lane c < 4 owns column c and walks the object's parts in index order.
__global__ __launch_bounds__(M3_THREADS) void k_metrics3d_object(const float *__restrict__ per_part, const int32_t *__restrict__ ptr,
                                                                  int P, int G, int has_pcds, float thr, float *__restrict__ per_object) {
    const int g = blockIdx.x * (M3_THREADS / 64) + (threadIdx.x >> 6), c = threadIdx.x & 63;
    if (g >= G || c >= 4) return;
    const int s = min(max(ptr[g], 0), P), e = min(max(ptr[g + 1], s), P);          // never past per_part
    float acc = 0.f;
    int hit = 0;
    for (int p = s; p < e; ++p) {
        const float v = per_part[(size_t)p * 4 + c];
        acc += v;
        hit += v < thr;
    }
    const float n = (float)(e - s);                        // no parts: 0 / 0 = NaN, torch's mean over nothing
    per_object[(size_t)g * 4 + c] = c < 3 ? acc / n : (has_pcds ? (float)hit / n : NAN);
}

}  // namespace
}  // namespace da

using namespace da;

extern "C" {

int da_metrics3d(int n_parts, int n_points, int n_objects, const float *pred, int ld_pred, const float *gt, int ld_gt,
                 const float *pcds, const int32_t *ptr, float thr, float *per_part, float *per_object, void *stream) {
    DA_REQUIRE(pred && gt && ptr && per_part && per_object, "da_metrics3d: null argument");
    DA_REQUIRE(n_parts > 0 && n_objects > 0 && (n_points > 0 || !pcds), "da_metrics3d: bad sizes (%d parts, %d points, %d objects)", n_parts,
               n_points, n_objects);
    DA_REQUIRE(ld_pred >= 7 && ld_gt >= 7, "da_metrics3d: pose rows hold 7 floats (ld_pred %d, ld_gt %d)", ld_pred, ld_gt);
    hipStream_t st = (hipStream_t)stream;
    k_metrics3d_part<<<n_parts, M3_THREADS, 0, st>>>(pred, ld_pred, gt, ld_gt, pcds, n_points, per_part);
    DA_LAUNCH_CHECK();
    const int waves = M3_THREADS / 64;
    k_metrics3d_object<<<(n_objects + waves - 1) / waves, M3_THREADS, 0, st>>>(per_part, ptr, n_parts, n_objects, pcds != nullptr, thr, per_object);
    DA_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
