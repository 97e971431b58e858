// MI355X (gfx950) fused predict kernel for kernel machines (SVM, kernel ridge).
//
//   K4k fused_predict_kernelmachine — per instance b, coalition sample s and
//       background row n:
//           row[j] = mask[b,s,g(j)] ? x[b,j] : bg[n,j]
//           kval[v] = exp(-gamma |row - sv[v]|^2)          (rbf)
//                   = (gamma row.sv[v] + coef0)^degree     (poly)
//           p  = act(intercept + alpha kval),  ey[b,s,:] = sum_n wbg[n] * p
//       Nothing but ey reaches global memory: neither the perturbation rows
//       nor the (rows, V) kernel matrix are ever formed.
//
// Fold, with k running over the varying groups (both the squared distance and
// the dot product are sums over coalition groups):
//     pre[s,n,v] = base[n,v] + sum_k mask[s,k] xp[b,v,k]
//                            - sum_k mask[s,k] bgp[n,v,k]
// The x term does not depend on n; bgp arrives already negated.
//
// Decomposition: one 256-thread workgroup (4 waves) owns (b, 64 consecutive
// samples).  The background rows are split into four contiguous ranges, one
// per wave; a wave walks its range in chunks of KM_NB rows and, inside a
// chunk, streams over ALL support-vector tiles of 16 for all 64 samples:
//     xt   = xp tile . mask^T                    once per (chunk, tile)
//     per row of the chunk:
//       acc  = xt + bgpn[n] tile . mask^T        (Mpad/4 MFMAs x 4 sample tiles)
//       kval = kernel(acc + base[n, tile])       (VALU, 4 values per lane)
//       z[n] += alpha tile . kval                (4 MFMAs x 4 sample tiles)
// The GEMM is taken transposed — support vectors are the MFMA rows, samples
// the columns — so that the kernel values, as they sit in the accumulator
// (row = (lane>>4)*4 + reg, col = lane&15), are directly the B operand of the
// contraction with alpha: step j of v_mfma_f32_16x16x4_f32 takes register j,
// whose lane quarter q holds support vector 4q+j, against the alpha fragment
// alpha[o = lane&15][tile*16 + 4q + j].  The sum over v therefore needs no
// cross-lane reduction, no LDS and no per-output registers: z is one
// accumulator tile (16 outputs x 16 samples) per row in flight and sample
// tile, whatever n_out is.  A wave owns whole background rows, so no wave
// ever waits on another inside the loop; the waves' partial sums over n are
// added through LDS in wave order at the very end.  No float atomics, fixed
// summation order: two launches are bit-identical.
//
// Every operand fragment fetched from global memory (L2-resident images,
// k-contiguous (v, Mpad) like the MLP kernel's) feeds 16 MFMAs, and the
// fragments of the next GEMM are fetched while the current one issues.  The
// mask tile is staged once in LDS (0/1, exact) and is read-only afterwards.
//
// KM_NB = 4 rows in flight: 64 accumulator registers for z next to 16 for the
// x term and 16 for the running tile; the x term then costs 16 of every 96
// MFMAs at Mpad = 64.
//
//   K4kp fused_predict_kernelmachine_pairs — the same kernel (EPI = 1) for a
//       one-vs-one multi-class SVM with K <= 6 classes: the output rows of z
//       are the P = K(K-1)/2 <= 15 pair decisions in libsvm order, and a
//       per-row epilogue turns them into K class scores before the weighted
//       background reduction:
//           act 3 (ovr)       votes + conf / (3 (|conf| + 1))
//           act 4 (coupling)  argmin p'Qp, sum p = 1, with Q built from the
//                             Platt pair probabilities
// The pair decisions of one sample sit in all four lane quarters (row =
// 4 (lane>>4) + reg), so a wave stages the 16 x 64 tile of one background row
// in its own quarter of ``red`` and reads it back with lane = sample (column
// reads at stride 64: conflict-free).  Store and load are ordered within the
// wave only — the waves own different numbers of rows, so there is no
// workgroup barrier inside the row loop.  Rows >= P (alpha = 0) are never
// read back.  Coupling solves the (K+1) x (K+1) KKT system
// [[Q, 1], [1', 0]] [p; lambda] = [0; 1] by LU with partial pivoting in
// registers: every index is a compile-time constant, the pivot is brought up
// by compare-and-swap of whole rows, and the trip counts depend on K alone
// (wave-uniform).  The K scores accumulate per lane; the cross-wave sum stays
// in wave order, so two launches are bit-identical here too.

#include <hip/hip_runtime.h>
#include <cstdint>

typedef __attribute__((ext_vector_type(4))) float km_f32x4;

#define KM_ROWS 64         // samples per workgroup (4 column tiles of 16)
#define KM_NW 4            // waves per workgroup
#define KM_NB 4            // background rows in flight per wave
#define KM_PAD 4           // mask row pad: 16 rows land on 16 distinct 16-B slots
#define KM_MAX_V 2048      // support vectors (padded)
#define KM_MAX_NOUT 8
#define KM_MAX_M 64        // varying groups
#define KM_MAX_DEGREE 8
#define KM_MAX_CLS 6       // classes of the one-vs-one epilogue (15 pair rows)

struct KmArgs {
    const uint8_t* masks;   // (B, S, M) raw coalition masks
    const float* xp;        // (B, Vpad, Mpad)  x part per support vector and group
    const float* bgpn;      // (N, Vpad, Mpad)  NEGATED background part
    const float* base;      // (N, Vpad)        whole-row term of bg[n]
    const float* alpha;     // (16, Vpad)       dual coefficients, zero-padded
    const float* icpt;      // (16)
    const float* wbg;       // (N)
    float* ey;              // (B, S, n_out)
    int B, S, M, N, Vpad, n_out, act, degree;
    float gamma, coef0;
    // one-vs-one epilogue (EPI = 1) only
    const float* prob_a;    // (16) Platt slope per pair
    const float* prob_b;    // (16) Platt offset per pair
    int K;                  // classes; n_out = K
};

template <int KCH>
__device__ __forceinline__ void km_load(
    const float* __restrict__ lanep, km_f32x4 (&a)[KCH])
{
#pragma unroll
    for (int kc = 0; kc < KCH; ++kc)
        a[kc] = *(const km_f32x4*)(lanep + kc * 16);
}

// acc[ct] += img tile (16 support vectors x Mpad, fragments in ``a``)
//            . mask tile ct (16 samples x Mpad, LDS)^T
// The four sample tiles are interleaved so that no MFMA waits on the one
// issued just before it.
template <int KCH>
__device__ __forceinline__ void km_gemm(
    const km_f32x4 (&a)[KCH], const float* mlane, km_f32x4 (&acc)[4])
{
    constexpr int MS = KCH * 16 + KM_PAD;
#pragma unroll
    for (int kc = 0; kc < KCH; ++kc) {
        km_f32x4 m[4];
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
            m[ct] = *(const km_f32x4*)(mlane + ct * 16 * MS + kc * 16);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int ct = 0; ct < 4; ++ct)
                acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                    a[kc][j], m[ct][j], acc[ct], 0, 0, 0);
    }
}

// Two workgroups per CU (two waves per SIMD): the compiler is held to 256
// registers, which it meets without scratch (252-254 at Mpad = 64).
template <int KCH, bool POLY, int EPI>
__global__ __launch_bounds__(KM_NW * 64, 2)
void fused_predict_km_kernel(KmArgs p)
{
    constexpr int MPAD = KCH * 16;
    constexpr int MS = MPAD + KM_PAD;
    constexpr int NTHR = KM_NW * 64;
    const int n_stiles = (p.S + KM_ROWS - 1) / KM_ROWS;
    const int b = blockIdx.x / n_stiles;
    const int s0 = (blockIdx.x % n_stiles) * KM_ROWS;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int arow = lane & 15;          // A row / B column within a tile
    const int akq = lane >> 4;           // k quarter; C/D row block

    extern __shared__ __attribute__((aligned(16))) unsigned char km_smem[];
    float* maskA = (float*)km_smem;              // 64 x MS  mask tile
    float* red = maskA + KM_ROWS * MS;           // KM_NW x 16 x 64  final sums

    // mask rows past S and pad columns are 0
    for (int idx = tid; idx < KM_ROWS * MPAD; idx += NTHR) {
        const int r = idx / MPAD;
        const int k = idx - r * MPAD;
        const int s = s0 + r;
        float v = 0.0f;
        if (s < p.S && k < p.M)
            v = (float)(p.masks[((size_t)b * p.S + s) * p.M + k] & 1);
        maskA[r * MS + k] = v;
    }
    __syncthreads();

    const int ntiles = p.Vpad / 16;
    const size_t istride = (size_t)p.Vpad * MPAD;
    const float* xpl = p.xp + (size_t)b * istride + arow * MPAD + akq * 4;
    const float* bgl = p.bgpn + arow * MPAD + akq * 4;
    const float* mlane = maskA + arow * MS + akq * 4;
    const int vq = akq * 4;              // this lane's 4 support vectors / outputs

    // this wave's contiguous share of the background rows
    const int nlo = (int)((long long)wave * p.N / KM_NW);
    const int nhi = (int)((long long)(wave + 1) * p.N / KM_NW);

    const km_f32x4 icv = *(const km_f32x4*)(p.icpt + vq);
    bool ovalid[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) ovalid[r] = vq + r < p.n_out;

    km_f32x4 eyacc[4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) eyacc[ct] = (km_f32x4){0, 0, 0, 0};
    // EPI = 1: the K class scores of sample ``lane``, summed over this
    // wave's rows (exact zeros for a wave without rows)
    float eyk[KM_MAX_CLS];
#pragma unroll
    for (int k = 0; k < KM_MAX_CLS; ++k) eyk[k] = 0.0f;

    km_f32x4 a_cur[KCH], a_nxt[KCH];
    if (nlo < nhi) km_load<KCH>(xpl, a_cur);

    for (int n0 = nlo; n0 < nhi; n0 += KM_NB) {
        const int cnt = min(KM_NB, nhi - n0);
        km_f32x4 z[KM_NB][4];
#pragma unroll
        for (int nb = 0; nb < KM_NB; ++nb)
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) z[nb][ct] = (km_f32x4){0, 0, 0, 0};

        for (int vt = 0; vt < ntiles; ++vt) {
            const size_t toff = (size_t)vt * 16 * MPAD;
            // a_cur holds the xp fragments of this tile; fetch the first
            // background row's while the x term issues
            km_load<KCH>(bgl + (size_t)n0 * istride + toff, a_nxt);
            const km_f32x4 al =
                *(const km_f32x4*)(p.alpha + (size_t)arow * p.Vpad + vt * 16 + vq);
            km_f32x4 xt[4];
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) xt[ct] = (km_f32x4){0, 0, 0, 0};
            km_gemm<KCH>(a_cur, mlane, xt);

#pragma unroll
            for (int nb = 0; nb < KM_NB; ++nb) {
                if (nb < cnt) {                       // wave-uniform
#pragma unroll
                    for (int kc = 0; kc < KCH; ++kc) a_cur[kc] = a_nxt[kc];
                    const km_f32x4 bs = *(const km_f32x4*)(
                        p.base + (size_t)(n0 + nb) * p.Vpad + vt * 16 + vq);
                    // what runs next: the next row of the chunk, the next
                    // tile's x part, or tile 0 for the next chunk (after the
                    // last chunk a harmless re-read of tile 0)
                    const float* nx;
                    if (nb + 1 < cnt)
                        nx = bgl + (size_t)(n0 + nb + 1) * istride + toff;
                    else if (vt + 1 < ntiles)
                        nx = xpl + toff + 16 * MPAD;
                    else
                        nx = xpl;
                    km_load<KCH>(nx, a_nxt);

                    km_f32x4 acc[4];
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct) acc[ct] = xt[ct];
                    km_gemm<KCH>(a_cur, mlane, acc);

                    // kernel values, in place: row = support vector vq + r
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const float pre = acc[ct][r] + bs[r];
                            float kv;
                            if (POLY) {
                                const float t = fmaf(p.gamma, pre, p.coef0);
                                kv = t;
                                for (int d = 1; d < p.degree; ++d) kv *= t;
                            } else {
                                kv = __expf(-p.gamma * pre);
                            }
                            acc[ct][r] = kv;
                        }
                    // z[o, s] += sum_v alpha[o, v] kval[v, s]
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int ct = 0; ct < 4; ++ct)
                            z[nb][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                                al[j], acc[ct][j], z[nb][ct], 0, 0, 0);
                }
            }
#pragma unroll
            for (int kc = 0; kc < KCH; ++kc) a_cur[kc] = a_nxt[kc];
        }

        if constexpr (EPI == 1) {
            // one-vs-one epilogue, one background row at a time
            float* stage = red + wave * (16 * 64);
            const int K = p.K;
#pragma nounroll
            for (int nb = 0; nb < cnt; ++nb) {
                km_f32x4 zz[4];
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) zz[ct] = z[0][ct];
#pragma unroll
                for (int q = 1; q < KM_NB; ++q)
                    if (nb == q) {                    // wave-uniform
#pragma unroll
                        for (int ct = 0; ct < 4; ++ct) zz[ct] = z[q][ct];
                    }
                const float wn = p.wbg[n0 + nb];
#pragma unroll
                for (int ct = 0; ct < 4; ++ct)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        stage[(vq + r) * 64 + ct * 16 + arow] = zz[ct][r] + icv[r];
                // the tile was written by other lanes of this wave
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                const float* fcol = stage + lane;     // f_p = fcol[p * 64]
                if (p.act == 3) {
                    float votes[KM_MAX_CLS], conf[KM_MAX_CLS];
#pragma unroll
                    for (int k = 0; k < KM_MAX_CLS; ++k) votes[k] = conf[k] = 0.0f;
                    int pp = 0;
#pragma unroll
                    for (int i = 0; i < KM_MAX_CLS; ++i)
#pragma unroll
                        for (int j = i + 1; j < KM_MAX_CLS; ++j)
                            if (j < K) {
                                const float f = fcol[pp * 64];
                                ++pp;
                                const bool neg = f < 0.0f;
                                votes[j] += neg ? 1.0f : 0.0f;
                                votes[i] += neg ? 0.0f : 1.0f;
                                conf[i] += f;
                                conf[j] -= f;
                            }
#pragma unroll
                    for (int k = 0; k < KM_MAX_CLS; ++k)
                        if (k < K)
                            eyk[k] += wn * (votes[k] + conf[k]
                                            / (3.0f * (fabsf(conf[k]) + 1.0f)));
                } else {
                    // augmented KKT system; variable k >= K is absent (its
                    // row and column are skipped everywhere), row / column 6
                    // is the multiplier, column 7 the right-hand side
                    constexpr int L = KM_MAX_CLS;
                    float A[L + 1][L + 2];
#pragma unroll
                    for (int r = 0; r <= L; ++r)
#pragma unroll
                        for (int c = 0; c <= L + 1; ++c) A[r][c] = 0.0f;
                    int pp = 0;
#pragma unroll
                    for (int i = 0; i < L; ++i)
#pragma unroll
                        for (int j = i + 1; j < L; ++j)
                            if (j < K) {
                                const float arg =
                                    fmaf(p.prob_a[pp], fcol[pp * 64], p.prob_b[pp]);
                                ++pp;
                                // r_ji is the sigmoid of the negated
                                // argument, not 1 - r_ij
                                float rij = __builtin_amdgcn_rcpf(1.0f + __expf(arg));
                                float rji = __builtin_amdgcn_rcpf(1.0f + __expf(-arg));
                                rij = fminf(fmaxf(rij, 1e-7f), 1.0f - 1e-7f);
                                rji = fminf(fmaxf(rji, 1e-7f), 1.0f - 1e-7f);
                                A[i][i] = fmaf(rji, rji, A[i][i]);
                                A[j][j] = fmaf(rij, rij, A[j][j]);
                                A[i][j] = A[j][i] = -rij * rji;
                            }
#pragma unroll
                    for (int k = 0; k < L; ++k)
                        if (k < K) A[k][L] = A[L][k] = 1.0f;
                    A[L][L + 1] = 1.0f;
                    float inv[L + 1];
#pragma unroll
                    for (int c = 0; c <= L; ++c) {
                        inv[c] = 0.0f;
                        if (c < K || c == L) {
#pragma unroll
                            for (int r = c + 1; r <= L; ++r)
                                if (r < K || r == L) {
                                    // first maximum wins, as in argmax
                                    const bool sw = fabsf(A[r][c]) > fabsf(A[c][c]);
#pragma unroll
                                    for (int k = c; k <= L + 1; ++k) {
                                        const float t = A[c][k];
                                        A[c][k] = sw ? A[r][k] : t;
                                        A[r][k] = sw ? t : A[r][k];
                                    }
                                }
                            inv[c] = 1.0f / A[c][c];
#pragma unroll
                            for (int r = c + 1; r <= L; ++r)
                                if (r < K || r == L) {
                                    const float m = A[r][c] * inv[c];
#pragma unroll
                                    for (int k = c + 1; k <= L + 1; ++k)
                                        A[r][k] = fmaf(-m, A[c][k], A[r][k]);
                                }
                        }
                    }
                    float x[L + 1];
#pragma unroll
                    for (int c = L; c >= 0; --c) {
                        x[c] = 0.0f;
                        if (c < K || c == L) {
                            float acc = A[c][L + 1];
#pragma unroll
                            for (int k = c + 1; k <= L; ++k)
                                acc = fmaf(-A[c][k], x[k], acc);
                            x[c] = acc * inv[c];
                        }
                    }
#pragma unroll
                    for (int k = 0; k < L; ++k)
                        if (k < K) eyk[k] = fmaf(wn, x[k], eyk[k]);
                }
                // the next row overwrites the tile other lanes just read
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
        } else {
            // activation over the outputs (registers r and lane quarters), then
            // the weighted background reduction, in row order
#pragma unroll
            for (int nb = 0; nb < KM_NB; ++nb) {
                if (nb < cnt) {
                    const float wn = p.wbg[n0 + nb];
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct) {
                        float zb[4], pr[4];
#pragma unroll
                        for (int r = 0; r < 4; ++r) zb[r] = z[nb][ct][r] + icv[r];
                        if (p.act == 2) {
                            float mx = -INFINITY;
#pragma unroll
                            for (int r = 0; r < 4; ++r)
                                mx = ovalid[r] ? fmaxf(mx, zb[r]) : mx;
                            mx = fmaxf(mx, __shfl_xor(mx, 16));
                            mx = fmaxf(mx, __shfl_xor(mx, 32));
                            float sum = 0.0f;
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                pr[r] = ovalid[r] ? __expf(zb[r] - mx) : 0.0f;
                                sum += pr[r];
                            }
                            sum += __shfl_xor(sum, 16);
                            sum += __shfl_xor(sum, 32);
                            const float inv = __builtin_amdgcn_rcpf(sum);
#pragma unroll
                            for (int r = 0; r < 4; ++r) pr[r] *= inv;
                        } else if (p.act == 1) {
#pragma unroll
                            for (int r = 0; r < 4; ++r)
                                pr[r] = __builtin_amdgcn_rcpf(1.0f + __expf(-zb[r]));
                        } else {
#pragma unroll
                            for (int r = 0; r < 4; ++r) pr[r] = zb[r];
                        }
#pragma unroll
                        for (int r = 0; r < 4; ++r) eyacc[ct][r] += wn * pr[r];
                    }
                }
            }
        }
    }

    if constexpr (EPI == 1) {
        // the four waves' class scores, added in wave order
#pragma unroll
        for (int k = 0; k < KM_MAX_CLS; ++k)
            red[wave * (16 * 64) + k * 64 + lane] = eyk[k];
        __syncthreads();
        const int K = p.K;
        for (int idx = tid; idx < KM_ROWS * K; idx += NTHR) {
            const int smp = idx / K;
            const int k = idx - smp * K;
            float sum = 0.0f;
#pragma unroll
            for (int w = 0; w < KM_NW; ++w)
                sum += red[w * (16 * 64) + k * 64 + smp];
            if (s0 + smp < p.S)
                p.ey[((size_t)b * p.S + s0 + smp) * K + k] = sum;
        }
        return;
    }

    // the four waves' sums over their rows, added in wave order
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            red[((wave * 4 + ct) * 4 + r) * 64 + lane] = eyacc[ct][r];
    __syncthreads();
    {
        const int ct = wave;             // wave w finishes sample tile w
        const int s = s0 + ct * 16 + arow;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float sum = 0.0f;
#pragma unroll
            for (int w = 0; w < KM_NW; ++w)
                sum += red[((w * 4 + ct) * 4 + r) * 64 + lane];
            if (ovalid[r] && s < p.S)
                p.ey[((size_t)b * p.S + s) * p.n_out + vq + r] = sum;
        }
    }
}

template <int KCH, int EPI>
static int launch_km_t(const KmArgs& a, int poly, hipStream_t stream)
{
    const size_t lds = sizeof(float)
        * ((size_t)KM_ROWS * (KCH * 16 + KM_PAD) + (size_t)KM_NW * 16 * 64);
    const long long n_stiles = (a.S + KM_ROWS - 1) / KM_ROWS;
    const long long nblk = (long long)a.B * n_stiles;
    if (nblk > 0x7fffffffLL) return -1;
    dim3 grid((unsigned)nblk), block(KM_NW * 64);
    if (poly)
        fused_predict_km_kernel<KCH, true, EPI><<<grid, block, lds, stream>>>(a);
    else
        fused_predict_km_kernel<KCH, false, EPI><<<grid, block, lds, stream>>>(a);
    return 0;
}

// Returns -1 outside the supported envelope: rbf or poly (degree 1-8),
// Vpad <= 2048 and a multiple of 16, n_out <= 8, M <= Mpad <= 64 with Mpad a
// multiple of 16.
extern "C" int launch_fused_predict_kernelmachine(
    const uint8_t* masks, const float* xp, const float* bgpn,
    const float* base, const float* alpha, const float* icpt,
    const float* wbg, float* ey, int B, int S, int M, int Mpad, int N,
    int Vpad, int n_out, int act, int kernel, float gamma, float coef0,
    int degree, hipStream_t stream)
{
    if (kernel != 0 && kernel != 1) return -1;
    if (kernel == 1 && (degree < 1 || degree > KM_MAX_DEGREE)) return -1;
    if (n_out < 1 || n_out > KM_MAX_NOUT) return -1;
    if (act < 0 || act > 2) return -1;
    if (M < 1 || M > Mpad || Mpad > KM_MAX_M || Mpad % 16 != 0) return -1;
    if (Vpad < 16 || Vpad > KM_MAX_V || Vpad % 16 != 0) return -1;
    if (B < 1 || S < 1 || N < 1) return -1;
    KmArgs a;
    a.masks = masks; a.xp = xp; a.bgpn = bgpn; a.base = base;
    a.alpha = alpha; a.icpt = icpt; a.wbg = wbg; a.ey = ey;
    a.B = B; a.S = S; a.M = M; a.N = N; a.Vpad = Vpad; a.n_out = n_out;
    a.act = act; a.degree = degree; a.gamma = gamma; a.coef0 = coef0;
    a.prob_a = nullptr; a.prob_b = nullptr; a.K = 0;
    switch (Mpad / 16) {
        case 1: return launch_km_t<1, 0>(a, kernel, stream);
        case 2: return launch_km_t<2, 0>(a, kernel, stream);
        case 3: return launch_km_t<3, 0>(a, kernel, stream);
        default: return launch_km_t<4, 0>(a, kernel, stream);
    }
}

// One-vs-one variant: alpha / icpt carry n_pairs = K(K-1)/2 pair rows, ey is
// (B, S, K).  Returns -1 outside the supported envelope: the limits above
// with, in place of the n_out rule, 3 <= K <= 6 and act 3 (ovr) or
// 4 (coupling).
extern "C" int launch_fused_predict_kernelmachine_pairs(
    const uint8_t* masks, const float* xp, const float* bgpn,
    const float* base, const float* alpha, const float* icpt,
    const float* prob_a, const float* prob_b, const float* wbg, float* ey,
    int B, int S, int M, int Mpad, int N, int Vpad, int n_classes,
    int n_pairs, int act, int kernel, float gamma, float coef0, int degree,
    hipStream_t stream)
{
    if (kernel != 0 && kernel != 1) return -1;
    if (kernel == 1 && (degree < 1 || degree > KM_MAX_DEGREE)) return -1;
    if (n_classes < 3 || n_classes > KM_MAX_CLS) return -1;
    if (n_pairs != n_classes * (n_classes - 1) / 2) return -1;
    if (act != 3 && act != 4) return -1;
    if (M < 1 || M > Mpad || Mpad > KM_MAX_M || Mpad % 16 != 0) return -1;
    if (Vpad < 16 || Vpad > KM_MAX_V || Vpad % 16 != 0) return -1;
    if (B < 1 || S < 1 || N < 1) return -1;
    KmArgs a;
    a.masks = masks; a.xp = xp; a.bgpn = bgpn; a.base = base;
    a.alpha = alpha; a.icpt = icpt; a.wbg = wbg; a.ey = ey;
    a.B = B; a.S = S; a.M = M; a.N = N; a.Vpad = Vpad; a.n_out = n_classes;
    a.act = act; a.degree = degree; a.gamma = gamma; a.coef0 = coef0;
    a.prob_a = prob_a; a.prob_b = prob_b; a.K = n_classes;
    switch (Mpad / 16) {
        case 1: return launch_km_t<1, 1>(a, kernel, stream);
        case 2: return launch_km_t<2, 1>(a, kernel, stream);
        case 3: return launch_km_t<3, 1>(a, kernel, stream);
        default: return launch_km_t<4, 1>(a, kernel, stream);
    }
}
