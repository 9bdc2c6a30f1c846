// The 3D assembly losses of loss_type="all" (puzzle_diff/model/utils_3d.py:585-890 as called at
// spatial_diffusion_3d_test_double_diffusion.py:500-562): trans_l2_loss, rot_cosine_loss and shape_cd_loss, forward and the
// gradient with respect to the predicted poses.  DESIGN.md 3i.
//
// shape_cd_loss is a K = 1 search both ways between the assembled shape under the predicted poses and under the target poses
// (two pytorch3d knn_points calls in the reference).  Here the poses are applied inside the kernels -- the posed clouds never
// reach memory -- and the padded parts are folded away: the reference fills them with points at (1e3, 1e3, 1e3) in both shapes
// and multiplies their distances by valids = 0, so only valid points are queries, and the candidates are the valid points of
// the other shape plus (when the shape has a padded slot) the single point (1e3, 1e3, 1e3).
//
// Pieces are rows of pred / gt [P, 7] (quaternion wxyz | translation); piece_map [P][2] = (shape, slot).  The pieces of one shape
// are consecutive rows with ascending slots (the order of the reference's x[valid_mask] = ...).  Indices are reported in the
// reference's padded frame: slot * N + point, within the shape.
#include <float.h>

#include "da_internal.h"

namespace da {
namespace {

constexpr int L3_THREADS = 256;
constexpr int L3_Q = 4;                          // queries per thread: one LDS read serves 4 x 4 pairs
constexpr int L3_QBLK = L3_THREADS * L3_Q;       // queries per workgroup
constexpr int L3_TILE = 1024;                    // candidates per LDS tile (12 KB)
constexpr int L3_MAXP = 64;                      // slots per shape (the slot set is one 64-bit mask)
constexpr float L3_FILL = 1e3f;                  // utils_3d.py:814,818
constexpr float L3_FAR = 1e18f;                  // tail of the last candidate group: never the nearest

// Rotation3D._process_zero_quat (utils_3d.py:174-181) then the matrix of pytorch3d quaternion_apply, q (0, v) conj(q) with NO
// normalisation: R = (w^2 - |u|^2) I + 2 u u^T + 2 w [u]x.  o[0..8] = R (row-major), o[9..11] = t.  Returns 1 when the
// quaternion was replaced by the identity (no gradient flows into it).
__device__ __forceinline__ int pose_eff(const float *__restrict__ pose, float *q) {
    const float w = pose[0], x = pose[1], y = pose[2], z = pose[3];
    const int zq = !(sqrtf(w * w + x * x + y * y + z * z) > 0.5f);
    q[0] = zq ? 1.f : w; q[1] = zq ? 0.f : x; q[2] = zq ? 0.f : y; q[3] = zq ? 0.f : z;
    return zq;
}
__device__ __forceinline__ int pose_xf(const float *__restrict__ pose, float *o) {
    float q[4];
    const int zq = pose_eff(pose, q);
    const float w = q[0], x = q[1], y = q[2], z = q[3];
    const float ww = w * w, xx = x * x, yy = y * y, zz = z * z;
    o[0] = ww + xx - yy - zz; o[1] = 2.f * (x * y - w * z); o[2] = 2.f * (x * z + w * y);
    o[3] = 2.f * (x * y + w * z); o[4] = ww - xx + yy - zz; o[5] = 2.f * (y * z - w * x);
    o[6] = 2.f * (x * z - w * y); o[7] = 2.f * (y * z + w * x); o[8] = ww - xx - yy + zz;
    o[9] = pose[4]; o[10] = pose[5]; o[11] = pose[6];
    return zq;
}
// explicit fma chains: the staging pass and the index pass of the search must produce the same bits
__device__ __forceinline__ void xf_apply(const float *o, float vx, float vy, float vz, float &X, float &Y, float &Z) {
    X = fmaf(o[2], vz, fmaf(o[1], vy, fmaf(o[0], vx, o[9])));
    Y = fmaf(o[5], vz, fmaf(o[4], vy, fmaf(o[3], vx, o[10])));
    Z = fmaf(o[8], vz, fmaf(o[7], vy, fmaf(o[6], vx, o[11])));
}
__device__ __forceinline__ float dist_sq(float ax, float ay, float az, float bx, float by, float bz) {
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    return fmaf(dz, dz, fmaf(dy, dy, dx * dx));
}

// Per shape b: info[b] = (first piece, valid pieces, first padded slot or -1, 0); slot_piece[b][slot] = piece or -1.
__global__ __launch_bounds__(256) void k_loss3d_prep(const int32_t *__restrict__ map, int P, int n_batch, int n_parts,
                                                     int32_t *__restrict__ info, int32_t *__restrict__ slot_piece) {
    for (int b = threadIdx.x; b < n_batch; b += 256) {
        int first = P, cnt = 0;
        unsigned long long mask = 0;
        for (int s = 0; s < n_parts; ++s) slot_piece[b * n_parts + s] = -1;
        for (int p = 0; p < P; ++p) {
            const int s = map[2 * p + 1];
            if (map[2 * p] != b || s < 0 || s >= n_parts) continue;
            first = min(first, p);
            ++cnt;
            mask |= 1ull << s;
            slot_piece[b * n_parts + s] = p;
        }
        cnt = min(cnt, min(n_parts, P - first));           // consecutive rows by contract; never past the arrays
        int fill = -1;
        for (int s = n_parts - 1; s >= 0; --s)
            if (!((mask >> s) & 1ull)) fill = s;
        info[4 * b] = cnt > 0 ? first : 0;
        info[4 * b + 1] = max(cnt, 0);
        info[4 * b + 2] = fill;
        info[4 * b + 3] = 0;
    }
}

// One direction of the search for 1024 queries of one shape: grid (ceil(n_parts N / 1024), n_batch, 2).  dir 0: queries under
// the predicted poses, candidates under the target poses; dir 1: the reverse.  Candidates are posed while they are staged into
// LDS as groups of four, x[4] y[4] z[4], so that three ds_read_b128 (a broadcast: every lane reads the same address) serve
// 4 candidates x 4 queries = 16 pairs per lane.  Per group and query: 4 x (3 sub, 1 mul, 2 fma), a 4-way min, and one
// compare + two selects that keep the best GROUP; the index inside the winning group is recovered after the loop by posing
// its four points again (same fma chain, same bits).  Strict '<' in ascending order: ties go to the lowest index.
__global__ __launch_bounds__(L3_THREADS) void k_loss3d_search(const float *__restrict__ pts, const float *__restrict__ pred,
                                                               const float *__restrict__ gt, const int32_t *__restrict__ map,
                                                               const int32_t *__restrict__ info, int N, int n_batch, size_t PN,
                                                               float *__restrict__ dist, int32_t *__restrict__ idx,
                                                               double *__restrict__ partial) {
    __shared__ float4 tile[L3_TILE / 4 * 3];
    __shared__ float xf[2][L3_MAXP][12];
    __shared__ double red[L3_THREADS / 64];
    const int tid = threadIdx.x, b = blockIdx.y, dir = blockIdx.z;
    const int start = info[4 * b], nv = info[4 * b + 1], fill_slot = info[4 * b + 2];
    const int nq = nv * N, q0 = blockIdx.x * L3_QBLK;
    double *pslot = partial + ((size_t)dir * n_batch + b) * gridDim.x + blockIdx.x;
    if (q0 >= nq) {
        if (tid == 0) *pslot = 0.0;
        return;
    }
    if (tid < 2 * nv) {                                    // xf[0]: the queries' poses, xf[1]: the candidates'
        const int side = tid >= nv, j = tid - side * nv;
        pose_xf(((side == 0) == (dir == 0) ? pred : gt) + (size_t)(start + j) * 7, xf[side][j]);
    }
    __syncthreads();
    const float *spts = pts + (size_t)start * N * 3;       // the shape's valid points, piece-major
    float qx[L3_Q], qy[L3_Q], qz[L3_Q], best[L3_Q];
    int bgrp[L3_Q];
#pragma unroll
    for (int k = 0; k < L3_Q; ++k) {
        const int q = min(q0 + k * L3_THREADS + tid, nq - 1);
        const float *v = spts + (size_t)q * 3;
        xf_apply(xf[0][q / N], v[0], v[1], v[2], qx[k], qy[k], qz[k]);
        best[k] = FLT_MAX;
        bgrp[k] = 0;
    }
    float *tf = reinterpret_cast<float *>(tile);
    for (int c0 = 0; c0 < nq; c0 += L3_TILE) {
        __syncthreads();
#pragma unroll
        for (int k = 0; k < L3_TILE / L3_THREADS; ++k) {
            const int ct = k * L3_THREADS + tid, c = c0 + ct;
            float X = L3_FAR, Y = L3_FAR, Z = L3_FAR;
            if (c < nq) {
                const float *v = spts + (size_t)c * 3;
                xf_apply(xf[1][c / N], v[0], v[1], v[2], X, Y, Z);
            }
            float *g = tf + (ct >> 2) * 12 + (ct & 3);
            g[0] = X; g[4] = Y; g[8] = Z;
        }
        __syncthreads();
        const int ng = (min(L3_TILE, nq - c0) + 3) >> 2, g0 = c0 >> 2;
#pragma unroll 2
        for (int g = 0; g < ng; ++g) {
            const float4 cx = tile[g * 3], cy = tile[g * 3 + 1], cz = tile[g * 3 + 2];
#pragma unroll
            for (int k = 0; k < L3_Q; ++k) {
                const float d0 = dist_sq(qx[k], qy[k], qz[k], cx.x, cy.x, cz.x);
                const float d1 = dist_sq(qx[k], qy[k], qz[k], cx.y, cy.y, cz.y);
                const float d2 = dist_sq(qx[k], qy[k], qz[k], cx.z, cy.z, cz.z);
                const float d3 = dist_sq(qx[k], qy[k], qz[k], cx.w, cy.w, cz.w);
                const float m = fminf(fminf(d0, d1), fminf(d2, d3));
                const bool lt = m < best[k];
                best[k] = lt ? m : best[k];
                bgrp[k] = lt ? g0 + g : bgrp[k];
            }
        }
    }
    double sum = 0.0;
#pragma unroll
    for (int k = 0; k < L3_Q; ++k) {
        const int q = q0 + k * L3_THREADS + tid;
        float bd = FLT_MAX;
        int bi = 0;
        for (int l = 0; l < 4; ++l) {
            const int c = bgrp[k] * 4 + l;
            if (c >= nq) break;
            const int j = c / N;
            const float *v = spts + (size_t)c * 3;
            float X, Y, Z;
            xf_apply(xf[1][j], v[0], v[1], v[2], X, Y, Z);
            const float d = dist_sq(qx[k], qy[k], qz[k], X, Y, Z);
            if (d < bd) { bd = d; bi = map[2 * (start + j) + 1] * N + (c - j * N); }
        }
        if (fill_slot >= 0) {                              // the padded parts of the other shape, as one candidate
            const float d = dist_sq(qx[k], qy[k], qz[k], L3_FILL, L3_FILL, L3_FILL);
            const int fi = fill_slot * N;
            if (d < bd || (d == bd && fi < bi)) { bd = d; bi = fi; }
        }
        if (q < nq) {
            dist[(size_t)dir * PN + (size_t)start * N + q] = bd;
            idx[(size_t)dir * PN + (size_t)start * N + q] = bi;
            sum += (double)bd;
        }
    }
    // fixed-order fp64 sum of the workgroup's distances (no atomics): lanes by shuffles, then the four waves in order
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_down(sum, o, 64);
    if ((tid & 63) == 0) red[tid >> 6] = sum;
    __syncthreads();
    if (tid == 0) *pslot = (red[0] + red[1]) + (red[2] + red[3]);
}

// out [3][n_batch] = per-shape (trans_l2_loss, shape_cd_loss, rot_cosine_loss), then out[3 n_batch + k] = weight k x the mean of
// row k over the shapes.  One workgroup; every sum runs serially in index order and in fp64 (a few thousand additions in all),
// so each output is the sum of the fp32 terms rounded ONCE.  shape_sum: fp64 scratch [3][n_batch].
__global__ __launch_bounds__(256) void k_loss3d_reduce(const float *__restrict__ pred, const float *__restrict__ gt,
                                                       const int32_t *__restrict__ info, const double *__restrict__ partial,
                                                       int nblk, int N, int n_batch, int n_parts, int terms, float w_trans,
                                                       float w_cd, float w_rot, double *__restrict__ shape_sum,
                                                       float *__restrict__ out) {
    for (int b = threadIdx.x; b < n_batch; b += 256) {
        const int start = info[4 * b], nv = info[4 * b + 1];
        double tr = 0.0, rot = 0.0, cd = 0.0;
        for (int j = 0; j < nv; ++j) {
            const float *a = pred + (size_t)(start + j) * 7, *c = gt + (size_t)(start + j) * 7;
            const double dx = (double)a[4] - c[4], dy = (double)a[5] - c[5], dz = (double)a[6] - c[6];
            tr += dx * dx + dy * dy + dz * dz;
            float q1[4], q2[4];
            pose_eff(a, q1);
            pose_eff(c, q2);
            rot += 1.0 - fabs((double)q1[0] * q2[0] + (double)q1[1] * q2[1] + (double)q1[2] * q2[2] + (double)q1[3] * q2[3]);
        }
        if (terms & 2) {
            const int live = (nv * N + L3_QBLK - 1) / L3_QBLK;
            double s0 = 0.0, s1 = 0.0;
            for (int k = 0; k < live; ++k) s0 += partial[(size_t)b * nblk + k];
            for (int k = 0; k < live; ++k) s1 += partial[((size_t)n_batch + b) * nblk + k];
            cd = (s0 + s1) / ((double)n_parts * (double)N);                  // torch.mean over P * N, padded slots counted
        }
        tr = (terms & 1) ? tr / (double)nv : 0.0;                            // _valid_mean: / valids.sum(1)
        rot = (terms & 4) ? rot / (double)nv : 0.0;
        shape_sum[b] = tr; shape_sum[n_batch + b] = cd; shape_sum[2 * n_batch + b] = rot;
        out[b] = (float)tr; out[n_batch + b] = (float)cd; out[2 * n_batch + b] = (float)rot;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        double s = 0.0;
        for (int b = 0; b < n_batch; ++b) s += shape_sum[threadIdx.x * n_batch + b];
        const float w = threadIdx.x == 0 ? w_trans : (threadIdx.x == 1 ? w_cd : w_rot);
        out[3 * n_batch + threadIdx.x] = (float)((double)w * s / (double)n_batch);
    }
}

// Gradient with respect to pred [P, 7]: one workgroup per piece.  The Chamfer term reaches the piece's posed points x = R(q) v + t
// (a) through their own matches (dir 0) and (b) through every target-side query of the shape whose match is one of them (dir 1:
// the workgroup scans its shape's match list).  With g = dL/dx per point, the piece needs only G = sum g and A = sum v g^T:
//   dt = G,  dw = 2 w tr A + 2 u . ax(A),  du = -2 tr(A) u + 2 A u + 2 A^T u + 2 w ax(A),  ax(A)_k = eps_kab A_ab.
// The twelve sums are reduced in a fixed order (lane shuffles, then the waves in order): bitwise reproducible.
__global__ __launch_bounds__(256) void k_loss3d_backward(const float *__restrict__ pts, const float *__restrict__ pred,
                                                         const float *__restrict__ gt, const int32_t *__restrict__ map,
                                                         const int32_t *__restrict__ info, const int32_t *__restrict__ slot_piece,
                                                         const int32_t *__restrict__ idx, const float *__restrict__ gout, int P,
                                                         int N, int n_batch, int n_parts, int terms, float *__restrict__ gpred) {
    __shared__ float red[4][12];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int b = map[2 * p], slot = map[2 * p + 1];
    if (b < 0 || b >= n_batch || slot < 0 || slot >= n_parts) {
        if (tid < 7) gpred[(size_t)p * 7 + tid] = 0.f;
        return;
    }
    const int start = info[4 * b], nv = info[4 * b + 1];
    const size_t PN = (size_t)P * N;
    float o1[12];
    const int zq = pose_xf(pred + (size_t)p * 7, o1);
    float acc[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) acc[e] = 0.f;
    if ((terms & 2) && p >= start && p < start + nv) {
        const float gcd = 2.f * gout[n_batch + b] / ((float)n_parts * (float)N);
        const float *pv = pts + (size_t)p * N * 3;
        auto add = [&](const float *v, float yx, float yy, float yz) {
            float X, Y, Z;
            xf_apply(o1, v[0], v[1], v[2], X, Y, Z);
            const float gx = gcd * (X - yx), gy = gcd * (Y - yy), gz = gcd * (Z - yz);
            acc[0] += v[0] * gx; acc[1] += v[0] * gy; acc[2] += v[0] * gz;
            acc[3] += v[1] * gx; acc[4] += v[1] * gy; acc[5] += v[1] * gz;
            acc[6] += v[2] * gx; acc[7] += v[2] * gy; acc[8] += v[2] * gz;
            acc[9] += gx; acc[10] += gy; acc[11] += gz;
        };
        for (int n = tid; n < N; n += 256) {               // (a) the piece's own queries
            const int j = idx[(size_t)p * N + n];
            const int s = j / N, nn = j - s * N;
            const int pc = (j >= 0 && s < n_parts) ? slot_piece[b * n_parts + s] : -1;
            float yx = L3_FILL, yy = L3_FILL, yz = L3_FILL;
            if (pc >= 0) {
                float o2[12];
                pose_xf(gt + (size_t)pc * 7, o2);
                const float *v2 = pts + ((size_t)pc * N + nn) * 3;
                xf_apply(o2, v2[0], v2[1], v2[2], yx, yy, yz);
            }
            add(pv + (size_t)n * 3, yx, yy, yz);
        }
        for (int i = tid; i < nv * N; i += 256) {          // (b) target-side queries matched to this piece
            const int j = idx[PN + (size_t)start * N + i];
            const int s = j / N;
            if (j < 0 || s != slot) continue;
            const int nn = j - s * N, jq = i / N;
            float o2[12], yx, yy, yz;
            pose_xf(gt + (size_t)(start + jq) * 7, o2);
            const float *v2 = pts + ((size_t)start * N + i) * 3;
            xf_apply(o2, v2[0], v2[1], v2[2], yx, yy, yz);
            add(pv + (size_t)nn * 3, yx, yy, yz);
        }
    }
#pragma unroll
    for (int e = 0; e < 12; ++e) {
        float s = acc[e];
        for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
        if ((tid & 63) == 0) red[tid >> 6][e] = s;
    }
    __syncthreads();
    if (tid != 0) return;
    float A[12];
    for (int e = 0; e < 12; ++e) A[e] = (red[0][e] + red[1][e]) + (red[2][e] + red[3][e]);
    float q[4], q2[4];
    pose_eff(pred + (size_t)p * 7, q);
    const int zq2 = pose_eff(gt + (size_t)p * 7, q2);
    (void)zq2;
    float g[7] = {0.f, 0.f, 0.f, 0.f, A[9], A[10], A[11]};
    if (!zq) {
        const float w = q[0], ux = q[1], uy = q[2], uz = q[3];
        const float trA = A[0] + A[4] + A[8];
        const float axx = A[5] - A[7], axy = A[6] - A[2], axz = A[1] - A[3];
        g[0] = 2.f * w * trA + 2.f * (ux * axx + uy * axy + uz * axz);
        const float Aux = A[0] * ux + A[1] * uy + A[2] * uz, Auy = A[3] * ux + A[4] * uy + A[5] * uz, Auz = A[6] * ux + A[7] * uy + A[8] * uz;
        const float Atx = A[0] * ux + A[3] * uy + A[6] * uz, Aty = A[1] * ux + A[4] * uy + A[7] * uz, Atz = A[2] * ux + A[5] * uy + A[8] * uz;
        g[1] = 2.f * (Aux + Atx - trA * ux + w * axx);
        g[2] = 2.f * (Auy + Aty - trA * uy + w * axy);
        g[3] = 2.f * (Auz + Atz - trA * uz + w * axz);
    }
    const float inv_nv = 1.f / (float)nv;
    if (terms & 1) {
        const float gt_ = 2.f * gout[b] * inv_nv;
        const float *a = pred + (size_t)p * 7, *c = gt + (size_t)p * 7;
        g[4] += gt_ * (a[4] - c[4]); g[5] += gt_ * (a[5] - c[5]); g[6] += gt_ * (a[6] - c[6]);
    }
    if ((terms & 4) && !zq) {
        const float dot = q[0] * q2[0] + q[1] * q2[1] + q[2] * q2[2] + q[3] * q2[3];
        const float sg = dot > 0.f ? 1.f : (dot < 0.f ? -1.f : 0.f);
        const float gr = -sg * gout[2 * n_batch + b] * inv_nv;
        for (int e = 0; e < 4; ++e) g[e] += gr * q2[e];
    }
    for (int e = 0; e < 7; ++e) gpred[(size_t)p * 7 + e] = g[e];
}

size_t ws_info_bytes(int n_batch, int n_parts) { return align_up((size_t)n_batch * (4 + n_parts) * sizeof(int32_t), 256); }
int search_blocks(int n_parts, int n_points) { return (int)(((long long)n_parts * n_points + L3_QBLK - 1) / L3_QBLK); }
size_t ws_partial_bytes(int n_batch, int n_parts, int n_points) { return align_up((size_t)2 * n_batch * search_blocks(n_parts, n_points) * sizeof(double), 256); }

int check_dims(const char *who, int n_pieces, int n_points, int n_batch, int n_parts, int terms) {
    DA_REQUIRE(n_pieces > 0 && n_points > 0 && n_batch > 0, "%s: bad sizes (%d pieces, %d points, %d shapes)", who, n_pieces, n_points, n_batch);
    DA_REQUIRE(n_parts > 0 && n_parts <= L3_MAXP, "%s: n_parts %d outside 1..%d", who, n_parts, L3_MAXP);
    DA_REQUIRE((long long)n_pieces <= (long long)n_batch * n_parts, "%s: %d pieces do not fit %d shapes of %d slots", who, n_pieces, n_batch, n_parts);
    DA_REQUIRE((long long)n_parts * n_points < (1ll << 30), "%s: n_parts * n_points too large", who);
    DA_REQUIRE(n_batch <= 65535, "%s: at most 65535 shapes", who);
    DA_REQUIRE(terms > 0 && terms < 8, "%s: terms is a mask of DA_LOSS3D_TRANS | _SHAPE_CD | _ROT", who);
    return 0;
}

}  // namespace
}  // namespace da

using namespace da;

extern "C" {

size_t da_loss3d_workspace_bytes(int n_batch, int n_parts, int n_points) {
    if (n_batch <= 0 || n_parts <= 0 || n_points <= 0) return 0;
    return ws_info_bytes(n_batch, n_parts) + ws_partial_bytes(n_batch, n_parts, n_points) + align_up((size_t)3 * n_batch * sizeof(double), 256);
}

int da_loss3d_forward(int n_pieces, int n_points, int n_batch, int n_parts, int terms, const float *pts, const float *pred,
                      const float *gt, const int32_t *piece_map, float w_trans, float w_shape_cd, float w_rot, float *dist,
                      int32_t *idx, float *out, void *workspace, size_t workspace_bytes, void *stream) {
    if (int rc = check_dims("da_loss3d_forward", n_pieces, n_points, n_batch, n_parts, terms)) return rc;
    DA_REQUIRE(pred && gt && piece_map && out && workspace, "da_loss3d_forward: null argument");
    DA_REQUIRE(!(terms & DA_LOSS3D_SHAPE_CD) || (pts && dist && idx), "da_loss3d_forward: the shape term needs pts, dist and idx");
    DA_REQUIRE(workspace_bytes >= da_loss3d_workspace_bytes(n_batch, n_parts, n_points), "da_loss3d_forward: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    int32_t *info = (int32_t *)workspace, *slot_piece = info + (size_t)4 * n_batch;
    double *partial = (double *)((char *)workspace + ws_info_bytes(n_batch, n_parts));
    double *shape_sum = (double *)((char *)partial + ws_partial_bytes(n_batch, n_parts, n_points));
    const int nblk = search_blocks(n_parts, n_points);
    k_loss3d_prep<<<1, 256, 0, st>>>(piece_map, n_pieces, n_batch, n_parts, info, slot_piece);
    DA_LAUNCH_CHECK();
    if (terms & DA_LOSS3D_SHAPE_CD) {
        k_loss3d_search<<<dim3(nblk, n_batch, 2), L3_THREADS, 0, st>>>(pts, pred, gt, piece_map, info, n_points, n_batch,
                                                                        (size_t)n_pieces * n_points, dist, idx, partial);
        DA_LAUNCH_CHECK();
    }
    k_loss3d_reduce<<<1, 256, 0, st>>>(pred, gt, info, partial, nblk, n_points, n_batch, n_parts, terms, w_trans, w_shape_cd, w_rot,
                                       shape_sum, out);
    DA_LAUNCH_CHECK();
    return 0;
}

int da_loss3d_backward(int n_pieces, int n_points, int n_batch, int n_parts, int terms, const float *pts, const float *pred,
                       const float *gt, const int32_t *piece_map, const int32_t *idx, const float *grad_out, float *grad_pred,
                       const void *workspace, size_t workspace_bytes, void *stream) {
    if (int rc = check_dims("da_loss3d_backward", n_pieces, n_points, n_batch, n_parts, terms)) return rc;
    DA_REQUIRE(pred && gt && piece_map && grad_out && grad_pred && workspace, "da_loss3d_backward: null argument");
    DA_REQUIRE(!(terms & DA_LOSS3D_SHAPE_CD) || (pts && idx), "da_loss3d_backward: the shape term needs pts and idx");
    DA_REQUIRE(workspace_bytes >= da_loss3d_workspace_bytes(n_batch, n_parts, n_points), "da_loss3d_backward: workspace too small");
    const int32_t *info = (const int32_t *)workspace, *slot_piece = info + (size_t)4 * n_batch;
    k_loss3d_backward<<<n_pieces, 256, 0, (hipStream_t)stream>>>(pts, pred, gt, piece_map, info, slot_piece, idx, grad_out, n_pieces,
                                                                 n_points, n_batch, n_parts, terms, grad_pred);
    DA_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
