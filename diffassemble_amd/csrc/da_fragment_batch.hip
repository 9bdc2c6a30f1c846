// A 3D Batch from fragment meshes: what the reference's dataset/breakingbad_dt.py :113-149 does per part on the host
// in fp64 numpy -- trimesh.sample.sample_surface, _recenter_pc, _rotate_pc, _shuffle_pc, the fp32 cast of _pad_data -- in two
// launches.  Every random draw (the face picks, the barycentric pairs, the turns, the point order) is made on the host and
// arrives as an argument.  All arithmetic is fp64 with contraction off, operation for operation what
// diffassemble_amd/fragment_batch.py::_loop_batch3d does, except for the ORDER of the two long sums (the running sum of the
// areas and the centroid), which is fixed here and sequential there.
//
// k_mesh_cum_area: one workgroup of 256 threads per input part.  The faces go in chunks of 256: thread t takes face
//   base + t, area = 0.5 * sqrt(|(v1 - v0) x (v2 - v0)|^2) (0 past the end), the chunk is scanned inclusively in LDS in eight
//   doubling steps between two buffers, cum[base + t] = carry + scan[t], carry <- carry + scan[255].  The order depends on
//   nothing but F: the same bits on every run.  Vertex indices are clamped to the part's range.
//
// k_fragment_batch: one workgroup of 256 threads per OUTPUT part, dynamic LDS = 3 N + 768 doubles.
//   sample  thread t takes the points t, t + 256, ...: pick = u_face * cum[F - 1], the first face with cum >= pick (bisection,
//           clamped to F - 1), (a, b) = u_len folded into the triangle, point = (a e1 + b e2) + v0, kept in LDS as X[N] | Y[N] |
//           Z[N] (struct of arrays: thread t writes X[t + 256 m], consecutive doubles per wave, no bank conflict), and summed
//           into the thread's partial centroid in that order.
//   centre  the 256 partials are reduced in LDS in eight halving steps (fixed order, no atomics), centroid = sum / N.
//   store   thread t takes the OUTPUT points t, t + 256, ...: q = perm[j] clamped to 0 .. N - 1, p = (X[q], Y[q], Z[q]) -
//           centroid, out = rot @ p, cast to fp32, three floats at pcds + 3 j: a wave writes 768 contiguous bytes.  The LDS reads
//           at q are a random gather (that is what a shuffle is); their bank conflicts were not measured.
//   small   thread 0 writes the part's row of x (fp32 of the quaternion of rot^T, made here as the host route makes it, and of the centroid)
//           and batch.
// A table entry that points outside the buffers writes nothing for its part.  Nothing crosses workgroups.
#include "da_common.h"

#pragma clang fp contract(off)

namespace da {
namespace {

constexpr int FB_THREADS = 256;
constexpr int FB_MAX_POINTS = 2048;                 // (3 * 2048 + 3 * 256) * 8 = 55 296 bytes of LDS <= the 64 KiB of a plain launch

struct PartRange {
    long long v0, nv, f0, nf;
};

// the vertex and face rows of input part s; false when the tables point outside the buffers
__device__ inline bool part_range(int s, const long long *__restrict__ vert_ptr, const long long *__restrict__ face_ptr, long long n_vertices,
                                  long long n_faces, PartRange &r) {
    r.v0 = vert_ptr[s];
    r.nv = vert_ptr[s + 1] - r.v0;
    r.f0 = face_ptr[s];
    r.nf = face_ptr[s + 1] - r.f0;
    return r.v0 >= 0 && r.nv >= 1 && r.nv <= n_vertices - r.v0 && r.nv <= 0x7fffffffLL && r.f0 >= 0 && r.nf >= 1 && r.nf <= n_faces - r.f0 &&
           r.nf <= 0x7fffffffLL;
}

struct Tri {
    double ox, oy, oz, ax, ay, az, bx, by, bz;      // v0, v1 - v0, v2 - v0
};

__device__ inline Tri load_tri(const double *__restrict__ vertices, const int32_t *__restrict__ faces, const PartRange &r, long long face) {
    const int32_t *f = faces + 3 * (r.f0 + face);
    const long long hi = r.nv - 1;
    const long long i0 = min(max((long long)f[0], 0LL), hi), i1 = min(max((long long)f[1], 0LL), hi), i2 = min(max((long long)f[2], 0LL), hi);
    const double *a = vertices + 3 * (r.v0 + i0), *b = vertices + 3 * (r.v0 + i1), *c = vertices + 3 * (r.v0 + i2);
    Tri t;
    t.ox = a[0]; t.oy = a[1]; t.oz = a[2];
    t.ax = b[0] - t.ox; t.ay = b[1] - t.oy; t.az = b[2] - t.oz;
    t.bx = c[0] - t.ox; t.by = c[1] - t.oy; t.bz = c[2] - t.oz;
    return t;
}

// The scalar-first unit quaternion of rot^T (rot row-major [9]): scipy's Rotation.from_matrix(rot.T).as_quat()[[3, 0, 1, 2]] =
// fragment_batch.py::_matrix_to_quat operation for operation -- the branch is the largest of the diagonal and the trace, the first
// of equals, so the sign is scipy's.  a[i][j] of the transpose is rot[3 j + i].
__device__ inline void quat_of_transpose(const double *__restrict__ R, double &qw, double &qx, double &qy, double &qz) {
    const double a00 = R[0], a01 = R[3], a02 = R[6], a10 = R[1], a11 = R[4], a12 = R[7], a20 = R[2], a21 = R[5], a22 = R[8];
    const double tr = (a00 + a11) + a22;
    int c = 0;
    double best = a00;
    if (a11 > best) { c = 1; best = a11; }
    if (a22 > best) { c = 2; best = a22; }
    if (tr > best) c = 3;
    double x, y, z, w;
    if (c == 0) {                                  // i, j, k = 0, 1, 2
        x = (1.0 - tr) + 2.0 * a00; y = a10 + a01; z = a20 + a02; w = a21 - a12;
    } else if (c == 1) {                           // i, j, k = 1, 2, 0
        y = (1.0 - tr) + 2.0 * a11; z = a21 + a12; x = a01 + a10; w = a02 - a20;
    } else if (c == 2) {                           // i, j, k = 2, 0, 1
        z = (1.0 - tr) + 2.0 * a22; x = a02 + a20; y = a12 + a21; w = a10 - a01;
    } else {
        x = a21 - a12; y = a02 - a20; z = a10 - a01; w = 1.0 + tr;
    }
    const double n = sqrt(((x * x + y * y) + z * z) + w * w);
    qw = w / n; qx = x / n; qy = y / n; qz = z / n;
}

__global__ __launch_bounds__(FB_THREADS) void k_mesh_cum_area(int n_parts, const double *__restrict__ vertices, long long n_vertices,
                                                               const int32_t *__restrict__ faces, long long n_faces,
                                                               const long long *__restrict__ vert_ptr, const long long *__restrict__ face_ptr,
                                                               double *__restrict__ cum) {
    __shared__ double scan[2][FB_THREADS];
    const int tid = threadIdx.x;
    PartRange r;
    if (!part_range(blockIdx.x, vert_ptr, face_ptr, n_vertices, n_faces, r)) return;     // uniform per workgroup
    double carry = 0.0;
    for (long long base = 0; base < r.nf; base += FB_THREADS) {
        const long long i = base + tid;
        double area = 0.0;
        if (i < r.nf) {
            const Tri t = load_tri(vertices, faces, r, i);
            const double cx = t.ay * t.bz - t.az * t.by, cy = t.az * t.bx - t.ax * t.bz, cz = t.ax * t.by - t.ay * t.bx;
            area = sqrt(cx * cx + cy * cy + cz * cz) * 0.5;
        }
        scan[0][tid] = area;
        __syncthreads();
        int cur = 0;
#pragma unroll
        for (int off = 1; off < FB_THREADS; off <<= 1) {
            double v = scan[cur][tid];
            if (tid >= off) v = scan[cur][tid - off] + v;
            scan[cur ^ 1][tid] = v;
            cur ^= 1;
            __syncthreads();
        }
        // eight steps: the result is back in scan[0]
        if (i < r.nf) cum[r.f0 + i] = carry + scan[cur][tid];
        carry = carry + scan[cur][FB_THREADS - 1];
        __syncthreads();                           // the next chunk overwrites scan[0]
    }
}

__global__ __launch_bounds__(FB_THREADS) void k_fragment_batch(int n_parts, int N, const double *__restrict__ vertices, long long n_vertices,
                                                                const int32_t *__restrict__ faces, long long n_faces,
                                                                const long long *__restrict__ vert_ptr, const long long *__restrict__ face_ptr,
                                                                const double *__restrict__ cum, const int32_t *__restrict__ parts,
                                                                const double *__restrict__ u_face, const double *__restrict__ u_len,
                                                                const double *__restrict__ rot,
                                                                const int32_t *__restrict__ perm, float *__restrict__ pcds,
                                                                float *__restrict__ x, long long *__restrict__ batch,
                                                                int32_t *__restrict__ face_index) {
    extern __shared__ double lds[];                // X[N] | Y[N] | Z[N] | red[3][256]
    double *X = lds, *Y = lds + N, *Z = lds + 2 * (size_t)N, *red = lds + 3 * (size_t)N;
    const int tid = threadIdx.x;
    const int k = blockIdx.x;
    const int s = parts[2 * (size_t)k], g = parts[2 * (size_t)k + 1];
    if (s < 0 || s >= n_parts) return;             // uniform per workgroup, before the first barrier
    PartRange r;
    if (!part_range(s, vert_ptr, face_ptr, n_vertices, n_faces, r)) return;
    const int nf = (int)r.nf;
    const double *cs = cum + r.f0;
    const double total = cs[nf - 1];
    const size_t row = (size_t)s * N;              // the draws belong to the input part
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int j = tid; j < N; j += FB_THREADS) {
        const double pick = u_face[row + j] * total;
        int lo = 0, hi = nf;                       // numpy.searchsorted(cum, pick, "left"): the first face with cum >= pick; a NaN pick
                                                   // (a non-finite vertex made the total NaN) finds the first NaN of cum, as there
        while (lo < hi) {
            const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
            const double c = cs[mid];
            if (c < pick || (pick != pick && c == c)) lo = mid + 1; else hi = mid;      // numpy orders NaN last
        }
        const int face = min(lo, nf - 1);
        const Tri t = load_tri(vertices, faces, r, face);
        double a = u_len[2 * (row + j)], b = u_len[2 * (row + j) + 1];
        if (a + b > 1.0) {
            a = fabs(a - 1.0);
            b = fabs(b - 1.0);
        }
        const double px = (t.ax * a + t.bx * b) + t.ox, py = (t.ay * a + t.by * b) + t.oy, pz = (t.az * a + t.bz * b) + t.oz;
        X[j] = px;
        Y[j] = py;
        Z[j] = pz;
        sx = sx + px;
        sy = sy + py;
        sz = sz + pz;
        if (face_index) face_index[(size_t)k * N + j] = face;
    }
    red[tid] = sx;
    red[FB_THREADS + tid] = sy;
    red[2 * FB_THREADS + tid] = sz;
    __syncthreads();
#pragma unroll
    for (int off = FB_THREADS / 2; off > 0; off >>= 1) {
        if (tid < off) {
            red[tid] = red[tid] + red[tid + off];
            red[FB_THREADS + tid] = red[FB_THREADS + tid] + red[FB_THREADS + tid + off];
            red[2 * FB_THREADS + tid] = red[2 * FB_THREADS + tid] + red[2 * FB_THREADS + tid + off];
        }
        __syncthreads();
    }
    const double cx = red[0] / (double)N, cy = red[FB_THREADS] / (double)N, cz = red[2 * FB_THREADS] / (double)N;
    const double *R = rot + 9 * (size_t)s;
    const double r00 = R[0], r01 = R[1], r02 = R[2], r10 = R[3], r11 = R[4], r12 = R[5], r20 = R[6], r21 = R[7], r22 = R[8];
    float *out = pcds + 3 * (size_t)k * N;
    for (int j = tid; j < N; j += FB_THREADS) {
        const int q = min(max(perm[row + j], 0), N - 1);
        const double px = X[q] - cx, py = Y[q] - cy, pz = Z[q] - cz;
        out[3 * (size_t)j] = (float)(r00 * px + r01 * py + r02 * pz);
        out[3 * (size_t)j + 1] = (float)(r10 * px + r11 * py + r12 * pz);
        out[3 * (size_t)j + 2] = (float)(r20 * px + r21 * py + r22 * pz);
    }
    if (tid == 0) {
        float *xr = x + 7 * (size_t)k;
        double qw, qx, qy, qz;
        quat_of_transpose(R, qw, qx, qy, qz);
        xr[0] = (float)qw;
        xr[1] = (float)qx;
        xr[2] = (float)qy;
        xr[3] = (float)qz;
        xr[4] = (float)cx;
        xr[5] = (float)cy;
        xr[6] = (float)cz;
        batch[k] = g;
    }
}

}  // namespace
}  // namespace da

using namespace da;

extern "C" int da_mesh_cum_area(int n_parts, const double *vertices, long long n_vertices, const int32_t *faces, long long n_faces,
                                const long long *vert_ptr, const long long *face_ptr, double *cum, void *stream) {
    DA_REQUIRE(vertices && faces && vert_ptr && face_ptr && cum, "da_mesh_cum_area: null argument");
    DA_REQUIRE(n_parts > 0 && n_vertices > 0 && n_faces > 0, "da_mesh_cum_area: bad sizes (%d parts, %lld vertices, %lld faces)", n_parts,
               n_vertices, n_faces);
    k_mesh_cum_area<<<(unsigned)n_parts, FB_THREADS, 0, (hipStream_t)stream>>>(n_parts, vertices, n_vertices, faces, n_faces, vert_ptr, face_ptr,
                                                                               cum);
    DA_LAUNCH_CHECK();
    return 0;
}

extern "C" int da_fragment_batch(int n_out, int n_parts, int n_points, const double *vertices, long long n_vertices, const int32_t *faces,
                                 long long n_faces, const long long *vert_ptr, const long long *face_ptr, const double *cum,
                                 const int32_t *parts, const double *u_face, const double *u_len, const double *rot,
                                 const int32_t *perm, float *pcds, float *x, long long *batch, int32_t *face_index, void *stream) {
    DA_REQUIRE(vertices && faces && vert_ptr && face_ptr && cum && parts && u_face && u_len && rot && perm && pcds && x && batch,
               "da_fragment_batch: null argument");
    DA_REQUIRE(n_out > 0 && n_parts > 0 && n_vertices > 0 && n_faces > 0,
               "da_fragment_batch: bad sizes (%d output parts, %d parts, %lld vertices, %lld faces)", n_out, n_parts, n_vertices, n_faces);
    DA_REQUIRE(n_points >= 1 && n_points <= FB_MAX_POINTS, "da_fragment_batch: n_points is 1 .. %d: 24 bytes of LDS per point (got %d)",
               FB_MAX_POINTS, n_points);
    DA_REQUIRE((long long)n_parts * n_points < (1ll << 31) && (long long)n_out * n_points < (1ll << 31),
               "da_fragment_batch: parts * n_points too large");
    const size_t lds_bytes = ((size_t)3 * n_points + 3 * FB_THREADS) * sizeof(double);
    k_fragment_batch<<<(unsigned)n_out, FB_THREADS, lds_bytes, (hipStream_t)stream>>>(n_parts, n_points, vertices, n_vertices, faces, n_faces,
                                                                                       vert_ptr, face_ptr, cum, parts, u_face, u_len, rot,
                                                                                       perm, pcds, x, batch, face_index);
    DA_LAUNCH_CHECK();
    return 0;
}
