// MI355X (gfx950) fused predict kernel for feed-forward (MLP) predictors.
//
//   K4m fused_predict_mlp — per instance b, coalition sample s and background
//       row n:
//           row[j] = mask[b,s,g(j)] ? x[b,j] : bg[n,j]
//           h1 = relu(W1 row + b1), further relu hidden layers,
//           p  = act(W_L h + b_L),  ey[b,s,:] = sum_n wbg[n] * p
//       Nothing but ey reaches global memory: the perturbation rows are never
//       formed (the first layer is folded over the varying groups, the same
//       algebra as the linear kernels' diff image) and the hidden activations
//       live in one LDS tile.
//
// First-layer fold, with k running over the varying groups:
//     pre1[s,n,:] = (base1[n,:] + sum_k mask[s,k] xpart1[b,k,:])
//                   - sum_k mask[s,k] bgpart1[n,k,:]
// The x term does not depend on n: it is computed once per workgroup and
// kept in accumulators; bgpart1 arrives already negated.
//
// Decomposition: one 512-thread workgroup (8 waves, two per SIMD) owns
// (b, 64 consecutive samples), loops over n, accumulates wbg[n]*p in
// registers and writes ey once — no float atomics, no partials, bitwise
// deterministic.  Inside a layer, wave w owns the output column tiles w and
// w+8 for ALL 64 rows, so each weight fragment fetched from global memory
// (L2-resident, shared by every workgroup) feeds four MFMAs; the 64 x Hpad
// result is held in accumulators and overwrites the activation tile in place
// between two barriers.  Weight fragments are fetched one k chunk ahead, and
// the first chunk of the next layer (or of the next n) is issued before the
// barriers so that its latency hides behind the store phase.  The output
// layer (n_out <= 8, padded to one 16-column tile, weights staged in LDS) is
// computed by waves 0-3 on 16 rows each, followed by the activation across
// the 16-lane column group and the weighted background reduction.
//
// Operand layouts are k-contiguous, (out, in_pad), for A (LDS) and B
// (global) alike, so one 16-byte load per lane feeds four f32 MFMAs
// (v_mfma_f32_16x16x4_f32, lane quarter q supplies k = 4q+j in step j) or
// one bf16 MFMA (v_mfma_f32_16x16x32_bf16).  In the bf16 variant the
// activations are rounded to bf16 when stored to LDS, all accumulation is
// f32, and the output layer takes a hi+lo split weight image so that it is
// f32-grade (the activations are exact in bf16).

#include <hip/hip_runtime.h>
#include <cstdint>

typedef __attribute__((ext_vector_type(4))) float mlp_f32x4;
typedef __attribute__((ext_vector_type(8))) __bf16 mlp_bf16x8;

#define MLP_ROWS 64        // samples per workgroup (4 row tiles of 16)
#define MLP_NW 8           // waves per workgroup
#define MLP_CI (16 / MLP_NW)   // column tiles per wave and layer
#define MLP_MAX_H 256      // widest hidden layer
#define MLP_MAX_HID 3      // hidden layers
#define MLP_MAX_NOUT 8
#define MLP_MAX_M 64       // varying groups

template <typename T> struct MlpTraits;

template <> struct MlpTraits<float> {
    static constexpr int KC = 16;   // k depth of one operand load
    static constexpr int KV = 4;    // elements per lane per load
    static constexpr int PAD = 4;   // row pad: 16 rows land on 16 distinct 16-B slots
    typedef mlp_f32x4 Vec;
    static __device__ __forceinline__ mlp_f32x4 mma(Vec a, Vec b, mlp_f32x4 c) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[j], c, 0, 0, 0);
        return c;
    }
    static __device__ __forceinline__ float from_f32(float v) { return v; }
};

template <> struct MlpTraits<__bf16> {
    static constexpr int KC = 32;
    static constexpr int KV = 8;
    static constexpr int PAD = 8;
    typedef mlp_bf16x8 Vec;
    static __device__ __forceinline__ mlp_f32x4 mma(Vec a, Vec b, mlp_f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ __bf16 from_f32(float v) { return (__bf16)v; }
};

struct MlpArgs {
    const uint8_t* masks;   // (B, S, M) raw coalition masks
    const void* xp1;        // (B, H1, Mpad)   x part of the first layer
    const void* bgp1n;      // (N, H1, Mpad)   NEGATED background part
    const float* base1;     // (N, H1)         W1 bg[n] + b1
    const void* hw[MLP_MAX_HID - 1];      // (H[l+1], H[l]) hidden weights
    const float* hb[MLP_MAX_HID - 1];     // (H[l+1])
    const void* wout;       // (nsplit, 16, H[last])
    const float* bout;      // (16)
    const float* wbg;       // (N)
    float* ey;              // (B, S, n_out)
    int B, S, M, Mpad, N, nhid;
    int H[MLP_MAX_HID];     // padded hidden widths
    int n_out, act, nsplit;
};

// First k chunk of this wave's column tiles of W ((out, Kpad), global).
template <typename T>
__device__ __forceinline__ void mlp_load_b0(
    const T* __restrict__ Wg, int Kpad, int nt, int wave, int arow, int akq,
    typename MlpTraits<T>::Vec (&bv)[MLP_CI])
{
    typedef typename MlpTraits<T>::Vec Vec;
    const T* wlane = Wg + (size_t)arow * Kpad + akq * MlpTraits<T>::KV;
#pragma unroll
    for (int ci = 0; ci < MLP_CI; ++ci) {
        const int ct = wave + MLP_NW * ci;             // wave-uniform
        if (ct < nt) bv[ci] = *(const Vec*)(wlane + (size_t)ct * 16 * Kpad);
        else bv[ci] = Vec{};
    }
}

// acc[ci][rt] += A(64 x Kpad, LDS) . W(ct-th 16 rows of (out, Kpad), global)^T
// for this wave's column tiles ct = wave + MLP_NW*ci < nt and the four row
// tiles.  ``bv`` holds k chunk 0 of W (mlp_load_b0, issued by the caller
// ahead of the barriers); the operands of chunk kc+KC are fetched while
// chunk kc's MFMAs issue.
template <typename T>
__device__ __forceinline__ void mlp_gemm(
    const T* A, int astride, int Kpad, const T* __restrict__ Wg, int nt,
    int wave, int arow, int akq, typename MlpTraits<T>::Vec (&bv)[MLP_CI],
    mlp_f32x4 (&acc)[MLP_CI][4])
{
    typedef MlpTraits<T> TR;
    typedef typename TR::Vec Vec;
    const T* alane = A + arow * astride + akq * TR::KV;
    const T* wlane = Wg + (size_t)arow * Kpad + akq * TR::KV;
    Vec a[4];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
        a[rt] = *(const Vec*)(alane + rt * 16 * astride);
    for (int kc = 0; kc < Kpad; kc += TR::KC) {
        const int kn = kc + TR::KC;
        Vec an[4], bn[MLP_CI];
        if (kn < Kpad) {
#pragma unroll
            for (int ci = 0; ci < MLP_CI; ++ci) {
                const int ct = wave + MLP_NW * ci;
                if (ct < nt)
                    bn[ci] = *(const Vec*)(wlane + (size_t)ct * 16 * Kpad + kn);
                else
                    bn[ci] = Vec{};
            }
#pragma unroll
            for (int rt = 0; rt < 4; ++rt)
                an[rt] = *(const Vec*)(alane + rt * 16 * astride + kn);
        }
#pragma unroll
        for (int ci = 0; ci < MLP_CI; ++ci) {
            const int ct = wave + MLP_NW * ci;
            if (ct < nt) {
#pragma unroll
                for (int rt = 0; rt < 4; ++rt)
                    acc[ci][rt] = TR::mma(a[rt], bv[ci], acc[ci][rt]);
            }
        }
        if (kn < Kpad) {
#pragma unroll
            for (int rt = 0; rt < 4; ++rt) a[rt] = an[rt];
#pragma unroll
            for (int ci = 0; ci < MLP_CI; ++ci) bv[ci] = bn[ci];
        }
    }
}

// relu(acc + bias) of the wave's column tiles into the activation tile.
// C/D map: col = lane & 15, row = (lane >> 4) * 4 + reg.
template <typename T>
__device__ __forceinline__ void mlp_store_relu(
    T* hbuf, int hstride, int nt, int wave, int arow, int akq,
    const mlp_f32x4 (&acc)[MLP_CI][4], const float (&bias)[MLP_CI])
{
#pragma unroll
    for (int ci = 0; ci < MLP_CI; ++ci) {
        const int ct = wave + MLP_NW * ci;
        if (ct < nt) {
#pragma unroll
            for (int rt = 0; rt < 4; ++rt)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    hbuf[(rt * 16 + akq * 4 + r) * hstride + ct * 16 + arow] =
                        MlpTraits<T>::from_f32(
                            fmaxf(acc[ci][rt][r] + bias[ci], 0.0f));
        }
    }
}

template <typename T>
__global__ __launch_bounds__(MLP_NW * 64)
void fused_predict_mlp_kernel(MlpArgs p)
{
    typedef MlpTraits<T> TR;
    typedef typename TR::Vec Vec;
    constexpr int NTHR = MLP_NW * 64;
    const int n_stiles = (p.S + MLP_ROWS - 1) / MLP_ROWS;
    const int b = blockIdx.x / n_stiles;
    const int s0 = (blockIdx.x % n_stiles) * MLP_ROWS;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int arow = lane & 15;          // A row / B column within a tile
    const int akq = lane >> 4;           // k quarter

    int hmax = p.H[0];
#pragma unroll
    for (int l = 1; l < MLP_MAX_HID; ++l)
        if (l < p.nhid) hmax = max(hmax, p.H[l]);
    const int klast = p.H[p.nhid - 1];

    extern __shared__ __attribute__((aligned(16))) unsigned char mlp_smem[];
    const int MS = p.Mpad + TR::PAD;
    const int HS = hmax + TR::PAD;
    const int WS = klast + TR::PAD;
    T* maskA = (T*)mlp_smem;             // 64 x MS   mask tile (0/1, exact)
    T* hbuf = maskA + MLP_ROWS * MS;     // 64 x HS   activation tile
    T* wo = hbuf + MLP_ROWS * HS;        // nsplit*16 x WS   output weights

    // ---- stage the mask tile and the output weights once ------------------
    // mask rows past S and pad columns are 0
    for (int idx = tid; idx < MLP_ROWS * p.Mpad; idx += NTHR) {
        const int r = idx / p.Mpad;
        const int k = idx - r * p.Mpad;
        const int s = s0 + r;
        float v = 0.0f;
        if (s < p.S && k < p.M)
            v = (float)(p.masks[((size_t)b * p.S + s) * p.M + k] & 1);
        maskA[r * MS + k] = TR::from_f32(v);
    }
    {
        const int vpr = klast / TR::KV;  // 16-byte vectors per weight row
        for (int idx = tid; idx < p.nsplit * 16 * vpr; idx += NTHR) {
            const int r = idx / vpr;
            const int c = idx - r * vpr;
            *(Vec*)(wo + r * WS + c * TR::KV) =
                *(const Vec*)((const T*)p.wout + (size_t)r * klast + c * TR::KV);
        }
    }
    __syncthreads();

    const int H1 = p.H[0];
    const int nt1 = H1 / 16;
    const T* bgp = (const T*)p.bgp1n;
    const size_t bgstride = (size_t)H1 * p.Mpad;

    // ---- x term of the first layer: independent of n ----------------------
    Vec bpre[MLP_CI];
    mlp_f32x4 xt[MLP_CI][4];
#pragma unroll
    for (int ci = 0; ci < MLP_CI; ++ci)
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) xt[ci][rt] = (mlp_f32x4){0, 0, 0, 0};
    {
        const T* xw = (const T*)p.xp1 + (size_t)b * bgstride;
        mlp_load_b0<T>(xw, p.Mpad, nt1, wave, arow, akq, bpre);
        mlp_gemm<T>(maskA, MS, p.Mpad, xw, nt1, wave, arow, akq, bpre, xt);
    }

    // hidden biases do not depend on n
    float hbias[MLP_MAX_HID - 1][MLP_CI];
#pragma unroll
    for (int l = 1; l < MLP_MAX_HID; ++l)
#pragma unroll
        for (int ci = 0; ci < MLP_CI; ++ci) {
            const int ct = wave + MLP_NW * ci;
            hbias[l - 1][ci] = (l < p.nhid && ct < p.H[l] / 16)
                ? p.hb[l - 1][ct * 16 + arow] : 0.0f;
        }

    const bool ovalid = arow < p.n_out;
    const float bo = p.bout[arow];
    mlp_f32x4 eyacc = (mlp_f32x4){0, 0, 0, 0};

    mlp_load_b0<T>(bgp, p.Mpad, nt1, wave, arow, akq, bpre);
    for (int n = 0; n < p.N; ++n) {
        mlp_f32x4 acc[MLP_CI][4];
        // ---- layer 1: (x term + base1[n]) - mask . bgpart1[n] -------------
        // base1[n] is needed only at the store: its load overlaps the GEMM
        float b1v[MLP_CI];
#pragma unroll
        for (int ci = 0; ci < MLP_CI; ++ci) {
            const int ct = wave + MLP_NW * ci;
            b1v[ci] = ct < nt1 ? p.base1[(size_t)n * H1 + ct * 16 + arow] : 0.0f;
#pragma unroll
            for (int rt = 0; rt < 4; ++rt) acc[ci][rt] = xt[ci][rt];
        }
        mlp_gemm<T>(maskA, MS, p.Mpad, bgp + (size_t)n * bgstride, nt1,
                    wave, arow, akq, bpre, acc);
        // first weight chunk of what runs next, issued ahead of the barriers
        if (p.nhid > 1)
            mlp_load_b0<T>((const T*)p.hw[0], H1, p.H[1] / 16,
                           wave, arow, akq, bpre);
        else if (n + 1 < p.N)
            mlp_load_b0<T>(bgp + (size_t)(n + 1) * bgstride, p.Mpad, nt1,
                           wave, arow, akq, bpre);
        __syncthreads();      // every wave is done reading the previous tile
        mlp_store_relu<T>(hbuf, HS, nt1, wave, arow, akq, acc, b1v);
        __syncthreads();

        // ---- further hidden layers, in place ------------------------------
#pragma unroll
        for (int l = 1; l < MLP_MAX_HID; ++l) {
            if (l < p.nhid) {
                const int kin = p.H[l - 1];
                const int ntl = p.H[l] / 16;
#pragma unroll
                for (int ci = 0; ci < MLP_CI; ++ci)
#pragma unroll
                    for (int rt = 0; rt < 4; ++rt)
                        acc[ci][rt] = (mlp_f32x4){0, 0, 0, 0};
                mlp_gemm<T>(hbuf, HS, kin, (const T*)p.hw[l - 1], ntl,
                            wave, arow, akq, bpre, acc);
                if (l == 1 && p.nhid > 2)
                    mlp_load_b0<T>((const T*)p.hw[1], p.H[1], p.H[2] / 16,
                                   wave, arow, akq, bpre);
                else if (n + 1 < p.N)
                    mlp_load_b0<T>(bgp + (size_t)(n + 1) * bgstride, p.Mpad,
                                   nt1, wave, arow, akq, bpre);
                __syncthreads();
                mlp_store_relu<T>(hbuf, HS, ntl, wave, arow, akq, acc,
                                  hbias[l - 1]);
                __syncthreads();
            }
        }

        // ---- output layer: waves 0-3, 16 rows each x one 16-column tile,
        //      both operands from LDS (wave-uniform branch, no barrier inside)
        mlp_f32x4 z = (mlp_f32x4){0, 0, 0, 0};
        if (wave < 4) {
            const T* alane = hbuf + (wave * 16 + arow) * HS + akq * TR::KV;
            for (int sp = 0; sp < p.nsplit; ++sp) {
                const T* wlane = wo + (sp * 16 + arow) * WS + akq * TR::KV;
                for (int kc = 0; kc < klast; kc += TR::KC) {
                    const Vec a = *(const Vec*)(alane + kc);
                    const Vec bw = *(const Vec*)(wlane + kc);
                    z = TR::mma(a, bw, z);
                }
            }
        }
        // activation across the output columns (lanes of a 16-lane group),
        // then the weighted background reduction
        const float wn = p.wbg[n];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float zb = z[r] + bo;
            float pr;
            if (p.act == 2) {
                float mx = ovalid ? zb : -INFINITY;
                mx = fmaxf(mx, __shfl_xor(mx, 1));
                mx = fmaxf(mx, __shfl_xor(mx, 2));
                mx = fmaxf(mx, __shfl_xor(mx, 4));
                mx = fmaxf(mx, __shfl_xor(mx, 8));
                const float e = ovalid ? __expf(zb - mx) : 0.0f;
                float sum = e;
                sum += __shfl_xor(sum, 1);
                sum += __shfl_xor(sum, 2);
                sum += __shfl_xor(sum, 4);
                sum += __shfl_xor(sum, 8);
                pr = e * __builtin_amdgcn_rcpf(sum);
            } else if (p.act == 1) {
                pr = __builtin_amdgcn_rcpf(1.0f + __expf(-zb));
            } else {
                pr = zb;
            }
            eyacc[r] += wn * pr;
        }
    }

#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int s = s0 + wave * 16 + akq * 4 + r;
        if (wave < 4 && ovalid && s < p.S)
            p.ey[((size_t)b * p.S + s) * p.n_out + arow] = eyacc[r];
    }
}

template <typename T>
static int launch_mlp_t(const MlpArgs& a, hipStream_t stream)
{
    typedef MlpTraits<T> TR;
    int hmax = 0;
    for (int l = 0; l < a.nhid; ++l) {
        if (a.H[l] <= 0 || a.H[l] > MLP_MAX_H || a.H[l] % TR::KC != 0) return -1;
        hmax = a.H[l] > hmax ? a.H[l] : hmax;
    }
    if (a.Mpad % TR::KC != 0) return -1;
    const size_t lds = sizeof(T)
        * ((size_t)MLP_ROWS * ((a.Mpad + TR::PAD) + (hmax + TR::PAD))
           + (size_t)a.nsplit * 16 * (a.H[a.nhid - 1] + TR::PAD));
    if (lds > 160 * 1024) return -1;
    if (lds > 48 * 1024) {
        if (hipFuncSetAttribute(
                reinterpret_cast<const void*>(&fused_predict_mlp_kernel<T>),
                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)
            != hipSuccess)
            return -2;
    }
    const long long n_stiles = (a.S + MLP_ROWS - 1) / MLP_ROWS;
    const long long nblk = (long long)a.B * n_stiles;
    if (nblk > 0x7fffffffLL) return -1;
    dim3 grid((unsigned)nblk), block(MLP_NW * 64);
    fused_predict_mlp_kernel<T><<<grid, block, lds, stream>>>(a);
    return 0;
}

// Returns -1 outside the supported envelope: 1-3 hidden layers of padded
// width <= 256, relu hidden activation, n_out <= 8, M <= Mpad <= 64.
extern "C" int launch_fused_predict_mlp(
    const uint8_t* masks, const void* xp1, const void* bgp1n,
    const float* base1, const void* const* hw, const float* const* hb,
    const int* H, int nhid, const void* wout, const float* bout,
    const float* wbg, float* ey, int B, int S, int M, int Mpad, int N,
    int n_out, int act, int hidden_act, int is_bf16, int nsplit,
    hipStream_t stream)
{
    if (nhid < 1 || nhid > MLP_MAX_HID) return -1;
    if (hidden_act != 0) return -1;                    // relu only
    if (n_out < 1 || n_out > MLP_MAX_NOUT) return -1;
    if (act < 0 || act > 2) return -1;
    if (M < 1 || M > Mpad || Mpad > MLP_MAX_M) return -1;
    if (nsplit < 1 || nsplit > 2) return -1;
    if (B < 1 || S < 1 || N < 1) return -1;
    MlpArgs a;
    a.masks = masks; a.xp1 = xp1; a.bgp1n = bgp1n; a.base1 = base1;
    for (int l = 0; l < MLP_MAX_HID - 1; ++l) {
        a.hw[l] = (l < nhid - 1) ? hw[l] : nullptr;
        a.hb[l] = (l < nhid - 1) ? hb[l] : nullptr;
    }
    for (int l = 0; l < MLP_MAX_HID; ++l) a.H[l] = (l < nhid) ? H[l] : 0;
    a.wout = wout; a.bout = bout; a.wbg = wbg; a.ey = ey;
    a.B = B; a.S = S; a.M = M; a.Mpad = Mpad; a.N = N; a.nhid = nhid;
    a.n_out = n_out; a.act = act; a.nsplit = nsplit;
    return is_bf16 ? launch_mlp_t<__bf16>(a, stream)
                   : launch_mlp_t<float>(a, stream);
}
