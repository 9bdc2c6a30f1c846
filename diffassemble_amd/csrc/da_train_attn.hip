// Attention backward of the training path over the edge list (the route of every graph the matrix-core kernels of
// da_train_dense.hip do not take, and of da_config.train_attn = 0).
//
// Works on the CSR graph for every graph type (complete puzzles, Exphander expanders, the exophormer virtual-node edges,
// multi-edges), with NO atomics: one kernel walks the incoming edges of each destination (dq, and the per-(node, head) term
// D = sum_e p_e dp_e), a second walks the outgoing edges of each source (dk, dv) -- the host supplies both CSR orientations.
//   p_e  = exp(a_e - m_i) / (sum + 1e-16)          (m_i, 1/(sum+1e-16) saved by the forward kernel)
//   dp_e = <dO_i, v_j>,  ds_e = p_e (dp_e - D_i)
//   dq_i = scale * sum_e ds_e k_j,  dk_j = scale * sum_e ds_e q_i,  dv_j = sum_e p_e dO_i
#include "da_train.h"

namespace da {

// Destination side: wave per destination node i, lane l holds the EPL = C / 8
// contiguous channels [l * EPL, (l + 1) * EPL) of the H*C-wide rows (8 lanes per head), exactly the
// decomposition of the forward kernel (da_attn_csr.hip).  Writes dq_i and the skip gradient into
// the fused [n, 4 HC] gradient of the projection, and D_i per head.
template <int EPL>
__global__ __launch_bounds__(256) void k_attn_bwd_dst(int n_nodes, const int32_t *__restrict__ row_ptr,
                                                      const int32_t *__restrict__ col_src, int H, int HC,
                                                      const float *__restrict__ qkvs, const float *__restrict__ d_o,
                                                      const float *__restrict__ stats, float *__restrict__ dY4,
                                                      float *__restrict__ Dd, float scale) {
    const int lane = threadIdx.x & 63;
    const int i = (int)(((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    if (i >= n_nodes) return;
    const size_t ld = (size_t)4 * HC;
    const int off = lane * EPL, head = lane >> 3;
    float q[EPL], g[EPL], a1[EPL], a2[EPL];
#pragma unroll
    for (int x = 0; x < EPL; ++x) {
        q[x] = qkvs[(size_t)i * ld + off + x] * scale;
        g[x] = d_o[(size_t)i * HC + off + x];
        a1[x] = a2[x] = 0.f;
    }
    const float m = stats[((size_t)i * H + head) * 2], inv = stats[((size_t)i * H + head) * 2 + 1];
    float D = 0.f;
    const int beg = row_ptr[i], end = row_ptr[i + 1];
    for (int e = beg; e < end; ++e) {
        const int j = col_src[e];
        const float *kp = qkvs + (size_t)j * ld + HC + off;
        const float *vp = kp + HC;
        float kk[EPL], vv[EPL];
#pragma unroll
        for (int x = 0; x < EPL; ++x) { kk[x] = kp[x]; vv[x] = vp[x]; }
        float s = 0.f, dp = 0.f;
#pragma unroll
        for (int x = 0; x < EPL; ++x) { s = fmaf(q[x], kk[x], s); dp = fmaf(g[x], vv[x], dp); }
        s += __shfl_xor(s, 1); dp += __shfl_xor(dp, 1);
        s += __shfl_xor(s, 2); dp += __shfl_xor(dp, 2);
        s += __shfl_xor(s, 4); dp += __shfl_xor(dp, 4);
        const float p = expf(s - m) * inv;
        const float pd = p * dp;
        D += pd;
#pragma unroll
        for (int x = 0; x < EPL; ++x) { a1[x] = fmaf(pd, kk[x], a1[x]); a2[x] = fmaf(p, kk[x], a2[x]); }
    }
#pragma unroll
    for (int x = 0; x < EPL; ++x) {
        dY4[(size_t)i * ld + off + x] = (a1[x] - D * a2[x]) * scale;
        dY4[(size_t)i * ld + 3 * (size_t)HC + off + x] = g[x];
    }
    if ((lane & 7) == 0) Dd[(size_t)i * H + head] = D;
}

// Source side: wave per source node j over its OUTGOING edges (out_ptr / out_dst = CSR by source).
template <int EPL>
__global__ __launch_bounds__(256) void k_attn_bwd_src(int n_nodes, const int32_t *__restrict__ out_ptr,
                                                      const int32_t *__restrict__ out_dst, int H, int HC,
                                                      const float *__restrict__ qkvs, const float *__restrict__ d_o,
                                                      const float *__restrict__ stats, const float *__restrict__ Dd,
                                                      float *__restrict__ dY4, float scale) {
    const int lane = threadIdx.x & 63;
    const int j = (int)(((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    if (j >= n_nodes) return;
    const size_t ld = (size_t)4 * HC;
    const int off = lane * EPL, head = lane >> 3;
    float kk[EPL], vv[EPL], dk[EPL], dv[EPL];
#pragma unroll
    for (int x = 0; x < EPL; ++x) {
        kk[x] = qkvs[(size_t)j * ld + HC + off + x];
        vv[x] = qkvs[(size_t)j * ld + 2 * (size_t)HC + off + x];
        dk[x] = dv[x] = 0.f;
    }
    const int beg = out_ptr[j], end = out_ptr[j + 1];
    for (int e = beg; e < end; ++e) {
        const int i = out_dst[e];
        float q[EPL], g[EPL];
#pragma unroll
        for (int x = 0; x < EPL; ++x) { q[x] = qkvs[(size_t)i * ld + off + x] * scale; g[x] = d_o[(size_t)i * HC + off + x]; }
        const float m = stats[((size_t)i * H + head) * 2], inv = stats[((size_t)i * H + head) * 2 + 1];
        const float D = Dd[(size_t)i * H + head];
        float s = 0.f, dp = 0.f;
#pragma unroll
        for (int x = 0; x < EPL; ++x) { s = fmaf(q[x], kk[x], s); dp = fmaf(g[x], vv[x], dp); }
        s += __shfl_xor(s, 1); dp += __shfl_xor(dp, 1);
        s += __shfl_xor(s, 2); dp += __shfl_xor(dp, 2);
        s += __shfl_xor(s, 4); dp += __shfl_xor(dp, 4);
        const float p = expf(s - m) * inv;
        const float ds = p * (dp - D);
#pragma unroll
        for (int x = 0; x < EPL; ++x) { dk[x] = fmaf(ds, q[x], dk[x]); dv[x] = fmaf(p, g[x], dv[x]); }
    }
#pragma unroll
    for (int x = 0; x < EPL; ++x) {
        dY4[(size_t)j * ld + HC + off + x] = dk[x];
        dY4[(size_t)j * ld + 2 * (size_t)HC + off + x] = dv[x];
    }
}

int launch_attn_bwd(const da_graph *g, int H, int C, const float *qkvs, const float *d_o, const float *stats,
                    float *Dd, float *dY4, hipStream_t st) {
    const int n = g->n_nodes, HC = H * C;
    const float scale = 1.0f / sqrtf((float)C);
    const int grid = (int)(((size_t)n * 64 + 255) / 256);
#define DA_BWD_CASE(E)                                                                                              \
    case E:                                                                                                         \
        k_attn_bwd_dst<E><<<grid, 256, 0, st>>>(n, g->row_ptr, g->col_src, H, HC, qkvs, d_o, stats, dY4, Dd, scale); \
        k_attn_bwd_src<E><<<grid, 256, 0, st>>>(n, g->out_ptr, g->out_dst, H, HC, qkvs, d_o, stats, Dd, dY4, scale); \
        break;
    switch (C / 8) {
        DA_BWD_CASE(1) DA_BWD_CASE(2) DA_BWD_CASE(3) DA_BWD_CASE(4) DA_BWD_CASE(5) DA_BWD_CASE(8) DA_BWD_CASE(13) DA_BWD_CASE(16) DA_BWD_CASE(18)
        default:
            set_error("attention backward: unsupported head width C=%d", C);
            return 1;
    }
#undef DA_BWD_CASE
    DA_LAUNCH_CHECK();
    return 0;
}

}  // namespace da
