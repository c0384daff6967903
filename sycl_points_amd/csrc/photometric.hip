// Photometric (intensity) term of the registration for gfx950: the per-point intensity gradients of a cloud and the
// linearisation / error of the intensity residual over a kNN result (sp_intensity_gradient, sp_photometric_linearize,
// sp_photometric_error; include/sycl_points_amd.h). The objective is the photometric part of Park, Zhou, Koltun, "Colored Point
// Cloud Registration Revisited" (ICCV 2017); the reference fetches intensities in its linearisation kernel and ignores them.
//
// Gradient (K5's sibling, one lane per point): with unit normal n and the neighbours j of the point's own kNN row,
//   u_j = (p_j - p_a) - ((p_j - p_a) . n) n,  M = sum u_j u_j^T + m^2 n n^T,  g = sum u_j (I_j - I_a),  d = M^-1 g,  d -= (d . n) n
// (a least-squares fit of the intensity over the tangent plane; m^2 n n^T makes M regular along n and keeps d tangent). A workgroup's
// index lists are staged through LDS in whole lines as in cov_kernel; what stays scattered is the k gathered points (16 B) and
// intensities (4 B) per lane. Output: one float4 per point (d.x, d.y, d.z, I_a), so that the linearisation gathers 16 bytes per
// correspondence; (0, 0, 0, NaN) marks a row without a gradient.
//
// Term (the shape of K11 / K12, one lane per point, grid stride): for source point s with q = T s and winner t
//   r = (I_t + d_t . (q - t)) - I_s,   J = d_t^T [-R S | R],  S = skew(s)      (twist and perturbation of sp_linearize.h)
// and the point adds rho J^T J (21), rho J^T r (6) and the robust error (1) in the kLinTerms order, rho = robust_weight(|r|).
// Algorithmic bytes per correspondence: 16 source point + 4 source intensity + 8 kNN entry + 16 target point + 16 target row = 60.
// The sums are block_reduce_store and reduce_rows_1024 (registration_device.h): a fixed tree, no float atomics, no workgroup waits
// for another; two launches give the same bytes.
// The arithmetic of both is one SP_HD function each, compiled for the device and for the host twins (sp_*_host): every
// multiply-add is an explicit fmaf / chain3 (-ffp-contract=off) and no library function is called (photometric_error_of), so a
// twin's rows are the device's bit for bit under every loss.
#include <cstring>

#include "registration_device.h"

namespace sp {
namespace {

SP_HD bool finite3(float x, float y, float z) { return fabsf(x) <= FLT_MAX && fabsf(y) <= FLT_MAX && fabsf(z) <= FLT_MAX; }

// The gradient row of point a; nbr: its k neighbour indices.
SP_HD float4 intensity_gradient_row(const float4* __restrict__ pts, const float4* __restrict__ nrm, const float* __restrict__ inten,
                                    unsigned n_pts, unsigned a, const int32_t* nbr, int k) {
    const float qnan = __builtin_nanf("");
    const float4 pa = pts[a], n = nrm[a];
    const float Ia = inten[a];
    float mxx = 0.0f, mxy = 0.0f, mxz = 0.0f, myy = 0.0f, myz = 0.0f, mzz = 0.0f;
    float gx = 0.0f, gy = 0.0f, gz = 0.0f;
    unsigned m = 0;
    for (int j = 0; j < k; ++j) {
        const int idx = nbr[j];
        if (idx < 0 || (unsigned)idx == a || (unsigned)idx >= n_pts) continue;  // (an index past the cloud: never dereferenced)
        const float4 pj = pts[idx];
        const float Ij = inten[idx];
        if (!(fabsf(Ij) <= FLT_MAX) || !finite3(pj.x, pj.y, pj.z)) continue;
        const float ex = pj.x - pa.x, ey = pj.y - pa.y, ez = pj.z - pa.z;
        const float en = chain3(ex, n.x, ey, n.y, ez, n.z);
        const float ux = fmaf(-en, n.x, ex), uy = fmaf(-en, n.y, ey), uz = fmaf(-en, n.z, ez);
        const float dI = Ij - Ia;
        mxx = fmaf(ux, ux, mxx); mxy = fmaf(ux, uy, mxy); mxz = fmaf(ux, uz, mxz);
        myy = fmaf(uy, uy, myy); myz = fmaf(uy, uz, myz); mzz = fmaf(uz, uz, mzz);
        gx = fmaf(ux, dI, gx); gy = fmaf(uy, dI, gy); gz = fmaf(uz, dI, gz);
        ++m;
    }
    if (m < 3u || !(fabsf(Ia) <= FLT_MAX) || !finite3(n.x, n.y, n.z)) return make_float4(0.0f, 0.0f, 0.0f, qnan);
    const float m2 = (float)(m * m);
    const float wx = m2 * n.x, wy = m2 * n.y, wz = m2 * n.z;
    const float a00 = fmaf(wx, n.x, mxx), a01 = fmaf(wx, n.y, mxy), a02 = fmaf(wx, n.z, mxz);
    const float a11 = fmaf(wy, n.y, myy), a12 = fmaf(wy, n.z, myz), a22 = fmaf(wz, n.z, mzz);
    // symmetric inverse by the adjugate, the form and the threshold of sp_linearize.h (eigen_utils::inverse)
    const float c00 = fmaf(a11, a22, -a12 * a12);
    const float c01 = fmaf(a02, a12, -a01 * a22);
    const float c02 = fmaf(a01, a12, -a02 * a11);
    const float det = fmaf(a00, c00, fmaf(a01, c01, a02 * c02));
    if (!(fabsf(det) >= 1e-6f)) return make_float4(0.0f, 0.0f, 0.0f, qnan);
    const float inv_det = 1.0f / det;
    const float i00 = c00 * inv_det, i01 = c01 * inv_det, i02 = c02 * inv_det;
    const float i11 = fmaf(a00, a22, -a02 * a02) * inv_det;
    const float i12 = fmaf(a01, a02, -a00 * a12) * inv_det;
    const float i22 = fmaf(a00, a11, -a01 * a01) * inv_det;
    float dx = chain3(i00, gx, i01, gy, i02, gz);
    float dy = chain3(i01, gx, i11, gy, i12, gz);
    float dz = chain3(i02, gx, i12, gy, i22, gz);
    const float dn = chain3(dx, n.x, dy, n.y, dz, n.z);
    dx = fmaf(-dn, n.x, dx); dy = fmaf(-dn, n.y, dy); dz = fmaf(-dn, n.z, dz);
    if (!finite3(dx, dy, dz)) return make_float4(0.0f, 0.0f, 0.0f, Ia);
    return make_float4(dx, dy, dz, Ia);
}

// ln(z) for finite z >= 1 from operations that round alike on the host and on the device (the exponent by bits, +, -, *, /, fmaf;
// the precedent is sp_atan2f): z = m 2^e with m in [sqrt(1/2), sqrt 2], ln m = 2 atanh(y), y = (m - 1) / (m + 1), |y| <= 0.1716, the
// series to y^11 (the next term is below 6e-11 of the sum), ln 2 split into a 16-bit head and its remainder. Within 2 ulp.
SP_HD float photometric_log(float z) {
    if (!(z <= FLT_MAX)) return z;  // inf, NaN
    const uint32_t b = __builtin_bit_cast(uint32_t, z);
    int e = (int)(b >> 23) - 127;
    float m = __builtin_bit_cast(float, (b & 0x007fffffu) | 0x3f800000u);  // [1, 2)
    if (m > 1.41421356f) { m *= 0.5f; ++e; }
    const float y = (m - 1.0f) / (m + 1.0f), y2 = y * y;
    float p = 1.0f / 11.0f;
    p = fmaf(p, y2, 1.0f / 9.0f);
    p = fmaf(p, y2, 1.0f / 7.0f);
    p = fmaf(p, y2, 1.0f / 5.0f);
    p = fmaf(p, y2, 1.0f / 3.0f);
    const float lm = 2.0f * fmaf(y * y2, p, y);
    constexpr float kLn2Hi = 0x1.62e4p-1f, kLn2Lo = 0x1.7f7d1cp-20f;  // ln 2 = hi + lo
    return fmaf((float)e, kLn2Hi, fmaf((float)e, kLn2Lo, lm));
}
// robust_error (sp_math.h) with the two library calls taken out, so that the host twin's error is the device's bit for bit under
// every loss: the Tukey cube by two products instead of powf(., 3), the Cauchy logarithm by photometric_log instead of logf. The
// same functions of r, a few ulp from robust_error's values; NONE, Huber and Geman-McClure call no library function and are
// robust_error itself.
template <int LOSS>
SP_HD float photometric_error_of(float r, float s) {
    if (LOSS == LOSS_TUKEY) {
        if (!(r <= s)) return s * s / 6.0f;
        const float c = 1.0f - ((r * r) / (s * s));
        return (s * s / 6.0f) * (1.0f - (c * c) * c);
    }
    if (LOSS == LOSS_CAUCHY) return 0.5f * s * s * photometric_log(1.0f + ((r * r) / (s * s)));
    return robust_error<LOSS>(r, s);
}

// What one correspondence adds: source point s with intensity Is, q = T s, winner t with its gradient row (d, I_t).
// ERR_ONLY: the robust error alone, into out[0].
template <int LOSS, bool ERR_ONLY, int NOUT>
SP_HD void photometric_terms(const Rigid& T, float sx, float sy, float sz, float Is, float tx, float ty, float tz, const float4& row,
                             float scale, float (&out)[NOUT]) {
    static_assert(NOUT == (ERR_ONLY ? 1 : kLinTerms), "28 terms, or the error alone");
    float qx, qy, qz;
    transform_point(T, sx, sy, sz, qx, qy, qz);
    const float ex = qx - tx, ey = qy - ty, ez = qz - tz;
    const float r = (row.w + chain3(row.x, ex, row.y, ey, row.z, ez)) - Is;
    const float rn = fabsf(r);
    if constexpr (ERR_ONLY) {
        out[0] = photometric_error_of<LOSS>(rn, scale);
    } else {
        const float (&R)[3][3] = T.R;
        // v = R^T d; J = [s x v | v]
        const float v0 = chain3(R[0][0], row.x, R[1][0], row.y, R[2][0], row.z);
        const float v1 = chain3(R[0][1], row.x, R[1][1], row.y, R[2][1], row.z);
        const float v2 = chain3(R[0][2], row.x, R[1][2], row.y, R[2][2], row.z);
        const float J[6] = {fmaf(sy, v2, -sz * v1), fmaf(sz, v0, -sx * v2), fmaf(sx, v1, -sy * v0), v0, v1, v2};
        const float w = robust_weight<LOSS>(rn, scale);
        float wJ[6];
#pragma unroll
        for (int a = 0; a < 6; ++a) wJ[a] = w * J[a];
        int e = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int c = a; c < 6; ++c) out[e++] = wJ[a] * J[c];
#pragma unroll
        for (int a = 0; a < 6; ++a) out[21 + a] = wJ[a] * r;
        out[27] = photometric_error_of<LOSS>(rn, scale);
    }
}

struct PhotoArgs {
    const float4* src;
    const float* src_i;
    const float4* tgt;
    const float4* rows;
    const int32_t* nn_idx;
    const float* nn_d2;
    unsigned n;
    float max_d2, scale;
};

// One point of either pass: false when it adds nothing (out untouched).
template <int LOSS, bool ERR_ONLY, int NOUT>
SP_HD bool photometric_point(const PhotoArgs& P, const Rigid& T, unsigned i, float (&out)[NOUT]) {
    const int idx = P.nn_idx[i];
    if (idx < 0 || P.nn_d2[i] > P.max_d2) return false;  // (the second test is the geometric kernel's: both terms see one set)
    const float4 row = P.rows[idx];
    const float Is = P.src_i[i];
    if (row.w != row.w || !(fabsf(Is) <= FLT_MAX)) return false;
    const float4 s = P.src[i], t = P.tgt[idx];
    photometric_terms<LOSS, ERR_ONLY>(T, s.x, s.y, s.z, Is, t.x, t.y, t.z, row, P.scale, out);
    return true;
}

__global__ __launch_bounds__(kBlock) void intensity_gradient_direct_kernel(const float4* __restrict__ pts, const float4* __restrict__ nrm,
                                                                           const float* __restrict__ inten, unsigned n,
                                                                           const int32_t* __restrict__ knn, int k,
                                                                           float4* __restrict__ rows) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    rows[i] = intensity_gradient_row(pts, nrm, inten, n, i, knn + (size_t)i * k, k);
}
// The index lists of the workgroup's 256 points are one contiguous k KB block: copied into LDS with 16-byte loads (cov_kernel's
// staging); the rows leave as 4 KB of consecutive 16-byte stores as they are. `knn` 16-byte aligned, LDS = k KB.
__global__ __launch_bounds__(kBlock) void intensity_gradient_kernel(const float4* __restrict__ pts, const float4* __restrict__ nrm,
                                                                    const float* __restrict__ inten, unsigned n,
                                                                    const int32_t* __restrict__ knn, int k, float4* __restrict__ rows) {
    extern __shared__ int4 s_stage[];
    int32_t* s_idx = reinterpret_cast<int32_t*>(s_stage);
    const unsigned t = threadIdx.x;
    const unsigned base = blockIdx.x * kBlock;
    const unsigned cnt = min((unsigned)kBlock, n - base);
    const unsigned total = cnt * (unsigned)k;
    const int32_t* g = knn + (size_t)base * k;  // (base * k * 4 bytes: a multiple of 1 KB)
    const int4* g4 = reinterpret_cast<const int4*>(g);
    for (unsigned e = t; e < total / 4; e += kBlock) s_stage[e] = g4[e];
    for (unsigned e = (total & ~3u) + t; e < total; e += kBlock) s_idx[e] = g[e];
    __syncthreads();
    if (t < cnt) rows[base + t] = intensity_gradient_row(pts, nrm, inten, n, base + t, s_idx + t * k, k);
}

template <int LOSS>
__global__ __launch_bounds__(kBlock) void photometric_linearize_kernel(PhotoArgs P, QueryPose pose, float* __restrict__ rows_out,
                                                                       float* __restrict__ partials) {
    const Rigid T = load_pose(pose);
    float acc[kAcc - 1];
#pragma unroll
    for (int e = 0; e < kAcc - 1; ++e) acc[e] = 0.0f;
    unsigned cnt = 0;
    for (unsigned i = blockIdx.x * kBlock + threadIdx.x; i < P.n; i += gridDim.x * kBlock) {
        float t[kLinTerms];
#pragma unroll
        for (int e = 0; e < kLinTerms; ++e) t[e] = 0.0f;
        if (photometric_point<LOSS, false>(P, T, i, t)) {
#pragma unroll
            for (int e = 0; e < kLinTerms; ++e) acc[e] += t[e];
            ++cnt;
        }
        if (rows_out) {  // (28 floats = 112 bytes per point: seven 16-byte stores)
            float4* const o = reinterpret_cast<float4*>(rows_out + (size_t)i * kLinTerms);
#pragma unroll
            for (int e = 0; e < kLinTerms / 4; ++e) o[e] = make_float4(t[4 * e], t[4 * e + 1], t[4 * e + 2], t[4 * e + 3]);
        }
    }
    block_reduce_store<kAcc - 1>(acc, cnt, partials + (size_t)blockIdx.x * kPartial);
}

template <int LOSS>
__global__ __launch_bounds__(kBlock) void photometric_error_kernel(PhotoArgs P, QueryPose pose, float* __restrict__ partials) {
    const Rigid T = load_pose(pose);
    float acc[1] = {0.0f};
    unsigned cnt = 0;
    for (unsigned i = blockIdx.x * kBlock + threadIdx.x; i < P.n; i += gridDim.x * kBlock) {
        float t[1];
        if (photometric_point<LOSS, true>(P, T, i, t)) {
            acc[0] += t[0];
            ++cnt;
        }
    }
    block_reduce_store<1>(acc, cnt, partials + (size_t)blockIdx.x * kPartial);
}

// final_reduce_kernel of registration.hip without its Gauss-Newton step: the same fixed tree over the partial rows
__global__ __launch_bounds__(kFinalThreads) void photometric_final_reduce_kernel(const float* __restrict__ partials, unsigned nblocks,
                                                                                 int nv, sp_linearized* __restrict__ out) {
    __shared__ float red[kFinalThreads / 32][kPartial];
    reduce_rows_1024(partials, nblocks, nv, red);
    if (threadIdx.x == 0) unpack_totals(red[0], nv, out);
}

int invalid_arg(const char* msg) {
    sp_set_error(msg);
    return SP_ERR_INVALID_ARGUMENT;
}
constexpr size_t kPhotoWorkspaceBytes = (size_t)kMaxBlocks * kPartial * sizeof(float);

unsigned photo_reduce_grid(size_t n) {
    unsigned g = div_up(n, kBlock);
    if (g > (unsigned)kMaxBlocks) g = kMaxBlocks;
    return g ? g : 1;
}

int check_gradient_args(const float* points, const float* normals, const float* intensities, size_t n, const int32_t* knn_idx,
                        size_t k, const float* rows_out) {
    if (k < 2) return invalid_arg("[intensity_gradient] k must be at least 2");
    if (k > (size_t)INT32_MAX / 4) return invalid_arg("[intensity_gradient] k is too large");
    if (n >= (1ull << 32)) return invalid_arg("[intensity_gradient] more than 2^32 points");
    if (n && (!points || !normals || !intensities || !knn_idx || !rows_out))
        return invalid_arg("[intensity_gradient] points, normals, intensities, knn_idx and rows_out must not be null");
    return SP_OK;
}

// what the four term entry points check alike, before any HIP call
int check_term_args(const float* src, const float* src_i, size_t n, const float* tgt, const float* rows, const int32_t* nn_idx,
                    const float* nn_d2, const float* T, const sp_photometric_params* p, const sp_linearized* out) {
    if (!p || !out || !T) return invalid_arg("[photometric] params, out and transT must not be null");
    if (n && (!src || !src_i || !tgt || !rows || !nn_idx || !nn_d2))
        return invalid_arg("[photometric] source points and intensities, target points and rows, nn_idx and nn_d2 must not be null");
    if (p->robust_type < SP_LOSS_NONE || p->robust_type > SP_LOSS_GEMAN_MCCLURE)
        return invalid_arg("[photometric] unknown robust loss type");
    if (p->robust_type != SP_LOSS_NONE && !(p->robust_scale > 0.0f))
        return invalid_arg("[photometric] robust_scale must be greater than zero when a robust loss is set");
    if (n >= (1ull << 32)) return invalid_arg("[photometric] more than 2^32 source points");
    return SP_OK;
}
int check_photo_workspace(const void* ws, size_t bytes) {
    if (!ws || bytes < kPhotoWorkspaceBytes || (reinterpret_cast<uintptr_t>(ws) & 15) != 0)
        return invalid_arg("[photometric] workspace null, misaligned (16 bytes) or too small (sp_photometric_workspace_bytes)");
    return SP_OK;
}
PhotoArgs make_photo_args(const float* src, const float* src_i, size_t n, const float* tgt, const float* rows, const int32_t* nn_idx,
                          const float* nn_d2, const sp_photometric_params* p) {
    PhotoArgs P;
    P.src = reinterpret_cast<const float4*>(src);
    P.src_i = src_i;
    P.tgt = reinterpret_cast<const float4*>(tgt);
    P.rows = reinterpret_cast<const float4*>(rows);
    P.nn_idx = nn_idx;
    P.nn_d2 = nn_d2;
    P.n = (unsigned)n;
    P.max_d2 = p->max_correspondence_distance * p->max_correspondence_distance;
    P.scale = p->robust_scale;
    return P;
}

int run_device(bool err_only, const float* src, const float* src_i, size_t n, const float* tgt, const float* rows, const int32_t* nn_idx,
               const float* nn_d2, const float* T, int T_dev, const sp_photometric_params* p, sp_linearized* out, float* rows_out,
               void* ws, size_t ws_bytes, hipStream_t st) {
    if (const int rc = check_term_args(src, src_i, n, tgt, rows, nn_idx, nn_d2, T, p, out); rc != SP_OK) return rc;
    if (const int rc = check_photo_workspace(ws, ws_bytes); rc != SP_OK) return rc;
    if (rows_out && (reinterpret_cast<uintptr_t>(rows_out) & 15) != 0) return invalid_arg("[photometric] rows_out must be 16-byte aligned");
    if (n == 0) return zero_async(out, sizeof(sp_linearized), st);
    const PhotoArgs P = make_photo_args(src, src_i, n, tgt, rows, nn_idx, nn_d2, p);
    const QueryPose pose = query_pose(T, T_dev);
    const unsigned grid = photo_reduce_grid(n);
    float* partials = static_cast<float*>(ws);
    const int rc = with_loss(p->robust_type, [&](auto L) {
        constexpr int loss = decltype(L)::value;
        if (err_only) photometric_error_kernel<loss><<<grid, kBlock, 0, st>>>(P, pose, partials);
        else photometric_linearize_kernel<loss><<<grid, kBlock, 0, st>>>(P, pose, rows_out, partials);
        return SP_OK;
    });
    if (rc != SP_OK) return rc;
    photometric_final_reduce_kernel<<<1, kFinalThreads, 0, st>>>(partials, grid, err_only ? 1 : kAcc - 1, out);
    return launch_status();
}

// The host twin: the same per-point function; the sums in chunks of 64 points, then over the chunks (any order is within the
// classical bound; this one keeps the error far below it).
template <int LOSS, bool ERR_ONLY>
void run_host_loss(const PhotoArgs& P, const Rigid& T, sp_linearized* out, float* rows_out) {
    constexpr int NV = ERR_ONLY ? 1 : kLinTerms;
    constexpr unsigned kChunk = 64;
    float tot[NV];
    for (int e = 0; e < NV; ++e) tot[e] = 0.0f;
    uint32_t cnt = 0;
    for (unsigned lo = 0; lo < P.n; lo += kChunk) {
        float part[NV];
        for (int e = 0; e < NV; ++e) part[e] = 0.0f;
        const unsigned hi = P.n - lo < kChunk ? P.n : lo + kChunk;
        for (unsigned i = lo; i < hi; ++i) {
            float t[NV];
            for (int e = 0; e < NV; ++e) t[e] = 0.0f;
            if (photometric_point<LOSS, ERR_ONLY>(P, T, i, t)) {
                for (int e = 0; e < NV; ++e) part[e] += t[e];
                ++cnt;
            }
            if (!ERR_ONLY && rows_out) std::memcpy(rows_out + (size_t)i * kLinTerms, t, sizeof t);
        }
        for (int e = 0; e < NV; ++e) tot[e] += part[e];
    }
    std::memset(out, 0, sizeof *out);
    if (ERR_ONLY) {
        out->error = tot[0];
    } else {
        int e = 0;
        for (int a = 0; a < 6; ++a)
            for (int c = a; c < 6; ++c) {
                out->H[a * 6 + c] = tot[e];
                out->H[c * 6 + a] = tot[e];
                ++e;
            }
        for (int a = 0; a < 6; ++a) out->b[a] = tot[21 + a];
        out->error = tot[NV - 1];
    }
    out->inlier = cnt;
    out->inlier_lo = (float)(cnt & 4095u);
    out->inlier_hi = (float)(cnt >> 12);
}
template <bool ERR_ONLY>
int run_host(const float* src, const float* src_i, size_t n, const float* tgt, const float* rows, const int32_t* nn_idx,
             const float* nn_d2, const float* T, const sp_photometric_params* p, sp_linearized* out, float* rows_out) {
    if (const int rc = check_term_args(src, src_i, n, tgt, rows, nn_idx, nn_d2, T, p, out); rc != SP_OK) return rc;
    const PhotoArgs P = make_photo_args(src, src_i, n, tgt, rows, nn_idx, nn_d2, p);
    const Rigid Tr = load_rigid_colmajor(T);
    switch (p->robust_type) {
        case SP_LOSS_NONE: run_host_loss<LOSS_NONE, ERR_ONLY>(P, Tr, out, rows_out); break;
        case SP_LOSS_HUBER: run_host_loss<LOSS_HUBER, ERR_ONLY>(P, Tr, out, rows_out); break;
        case SP_LOSS_TUKEY: run_host_loss<LOSS_TUKEY, ERR_ONLY>(P, Tr, out, rows_out); break;
        case SP_LOSS_CAUCHY: run_host_loss<LOSS_CAUCHY, ERR_ONLY>(P, Tr, out, rows_out); break;
        default: run_host_loss<LOSS_GEMAN_MCCLURE, ERR_ONLY>(P, Tr, out, rows_out); break;
    }
    return SP_OK;
}

}  // namespace
}  // namespace sp

extern "C" int sp_intensity_gradient(const float* points, const float* normals, const float* intensities, size_t n,
                                     const int32_t* knn_idx, size_t k, float* rows_out, void* stream) {
    using namespace sp;
    if (const int rc = check_gradient_args(points, normals, intensities, n, knn_idx, k, rows_out); rc != SP_OK) return rc;
    if (n == 0) return SP_OK;
    const float4* p = reinterpret_cast<const float4*>(points);
    const float4* nr = reinterpret_cast<const float4*>(normals);
    float4* r = reinterpret_cast<float4*>(rows_out);
    if (k <= 64 && (reinterpret_cast<uintptr_t>(knn_idx) & 15) == 0)
        intensity_gradient_kernel<<<div_up(n, kBlock), kBlock, (size_t)kBlock * 4 * k, as_stream(stream)>>>(p, nr, intensities, (unsigned)n,
                                                                                                             knn_idx, (int)k, r);
    else
        intensity_gradient_direct_kernel<<<div_up(n, kBlock), kBlock, 0, as_stream(stream)>>>(p, nr, intensities, (unsigned)n, knn_idx,
                                                                                              (int)k, r);
    return launch_status();
}

extern "C" int sp_intensity_gradient_host(const float* points, const float* normals, const float* intensities, size_t n,
                                          const int32_t* knn_idx, size_t k, float* rows_out) {
    using namespace sp;
    if (const int rc = check_gradient_args(points, normals, intensities, n, knn_idx, k, rows_out); rc != SP_OK) return rc;
    const float4* p = reinterpret_cast<const float4*>(points);
    const float4* nr = reinterpret_cast<const float4*>(normals);
    for (size_t i = 0; i < n; ++i) {
        const float4 row = intensity_gradient_row(p, nr, intensities, (unsigned)n, (unsigned)i, knn_idx + i * k, (int)k);
        std::memcpy(rows_out + 4 * i, &row, sizeof row);
    }
    return SP_OK;
}

extern "C" size_t sp_photometric_workspace_bytes(size_t) { return sp::kPhotoWorkspaceBytes; }

extern "C" int sp_photometric_linearize(const float* src_points, const float* src_intensities, size_t n, const float* tgt_points,
                                        const float* tgt_rows, const int32_t* nn_idx, const float* nn_d2, const float* transT,
                                        int transT_on_device, const sp_photometric_params* params, sp_linearized* out,
                                        float* rows_out_opt, void* workspace, size_t workspace_bytes, void* stream) {
    return sp::run_device(false, src_points, src_intensities, n, tgt_points, tgt_rows, nn_idx, nn_d2, transT, transT_on_device, params,
                          out, rows_out_opt, workspace, workspace_bytes, sp::as_stream(stream));
}
extern "C" int sp_photometric_error(const float* src_points, const float* src_intensities, size_t n, const float* tgt_points,
                                    const float* tgt_rows, const int32_t* nn_idx, const float* nn_d2, const float* transT,
                                    int transT_on_device, const sp_photometric_params* params, sp_linearized* out, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    return sp::run_device(true, src_points, src_intensities, n, tgt_points, tgt_rows, nn_idx, nn_d2, transT, transT_on_device, params,
                          out, nullptr, workspace, workspace_bytes, sp::as_stream(stream));
}
extern "C" int sp_photometric_linearize_host(const float* src_points, const float* src_intensities, size_t n, const float* tgt_points,
                                             const float* tgt_rows, const int32_t* nn_idx, const float* nn_d2, const float* transT,
                                             const sp_photometric_params* params, sp_linearized* out, float* rows_out_opt) {
    return sp::run_host<false>(src_points, src_intensities, n, tgt_points, tgt_rows, nn_idx, nn_d2, transT, params, out, rows_out_opt);
}
extern "C" int sp_photometric_error_host(const float* src_points, const float* src_intensities, size_t n, const float* tgt_points,
                                         const float* tgt_rows, const int32_t* nn_idx, const float* nn_d2, const float* transT,
                                         const sp_photometric_params* params, sp_linearized* out) {
    return sp::run_host<true>(src_points, src_intensities, n, tgt_points, tgt_rows, nn_idx, nn_d2, transT, params, out, nullptr);
}
