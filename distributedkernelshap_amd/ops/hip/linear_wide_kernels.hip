// CDNA4 (gfx950) fused linear predict for 3..16 outputs (multi-class softmax).
//
//   K4l fused_predict_linear_wide
//
//   ey[b,s,o] = sum_n wbg[n] * act( base[o,n]
//                                   + sum_k mask[b,s,k] * diff[b,o,k,n] )
//
// Same maths, operands and MFMA orientation as fused_predict_linear (K3-K6 in
// kshap_kernels.hip): v_mfma_f32_16x16x4_f32 with A = 16 sample rows x 4 k,
// B = 4 k x 16 background columns, one fp32 accumulator tile per class, so the
// softmax over classes is register-local and only the weighted sum over n
// crosses lanes.  What differs is the decomposition.  The one-tile kernel
// stages the whole per-instance image OIMG x Mpad x NSTRIDE in LDS; at 16
// images x 64 groups x 128 columns that is 512 KiB.  Here
//
//   * the COLUMN TILE is the outer loop: one 16-column slice of the image,
//     n_out x Mpad x 16 fp32 (<= 64 KiB), is staged at a time and reused by
//     every wave and every s-sub-tile of the workgroup;
//   * a workgroup is 8 waves and owns (b, 512 samples) = 4 sub-tiles of 128
//     rows, so one workgroup per CU (the 16-class, 64-group worst case) still
//     keeps two waves on every SIMD;
//   * the slice layout is [k/4][o][k%4][16]: the four k-rows one MFMA reads
//     are 64 consecutive words (conflict-free ds_read_b32), the class offset
//     is a compile-time immediate, the k step one add;
//   * the A operand (0/1 masks) is read from global once, packed to one bit
//     per k step and lane (<= 16 bits per sub-tile, 64 bits a lane) and
//     expanded in-register for every column tile;
//   * per-sample running sums over the column tiles live in LDS,
//     sums[512][NOUTP].  After the 16-lane reduction every lane of a row
//     group holds the sum; lane (arow == o) keeps class o, so each (s, o) cell
//     has exactly one owner thread for the whole kernel: no atomics, no
//     barrier on the sums, a fixed summation order (column tiles ascending).
//
// Pad classes n_out <= o < NOUTP are predicated out with the wave-uniform
// n_out: their images are never staged, multiplied or reduced, so whatever the
// pad images hold cannot reach an output.
//
// Template params: NOUTP in {4,8,12,16} (classes padded to a multiple of 4);
// ACT 0 = none, 1 = sigmoid, 2 = softmax over the n_out real classes.
#include <hip/hip_runtime.h>

#include <cstdint>

#define LW_THREADS 512     // 8 waves
#define LW_S_SUB 128       // rows per sub-tile (8 waves x 16)
#define LW_NSUB 4
#define LW_S_TILE (LW_NSUB * LW_S_SUB)
#define LW_MAX_MPAD 64
#define LW_MAX_NPAD 512
#define LW_MAX_NOUT 16

typedef __attribute__((ext_vector_type(4))) float lw_f32x4;

// class o is real.  NOUTP is n_out rounded up to a multiple of 4, so only the
// last three classes of an instantiation need the run-time (wave-uniform)
// test.  With a run-time test on every class hipcc duplicates the epilogue per
// class count and the NOUTP = 8 instantiations spill to scratch.
#define LW_REAL(o) ((o) < NOUTP - 3 || (o) < n_out)

namespace {

__device__ __forceinline__ float lw_rcp(float x) {   // v_rcp_f32, 1 ulp
    return __builtin_amdgcn_rcpf(x);
}

// sum over the 16 lanes of a DPP row; every lane of the row gets the total.
// quad xor 1, quad xor 2, then the 8- and 16-lane mirrors (the operands of
// each mirror step are already uniform over the mirrored halves).
__device__ __forceinline__ float lw_row16_sum(float v) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(
        0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(
        0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(
        0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(
        0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true));
    return v;
}

}  // namespace

template <int NOUTP, int ACT>
__global__ __launch_bounds__(LW_THREADS)
void fused_predict_linear_wide_kernel(
    const uint8_t* __restrict__ masksU, // (B, S, M) raw coalition masks
    const float* __restrict__ diff,     // (B, NOUTP, Mpad, Npad)
    const float* __restrict__ base,     // (NOUTP, Npad)
    const float* __restrict__ wbg,      // (Npad)  0 for padding cols
    float* __restrict__ ey,             // (B, S, n_out)
    int B, int S, int M, int Mpad, int Npad, int n_out)
{
    const int n_stiles = (S + LW_S_TILE - 1) / LW_S_TILE;
    const int b = blockIdx.x / n_stiles;
    const int s0 = (blockIdx.x % n_stiles) * LW_S_TILE;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;           // 0..7
    const int arow = lane & 15;          // A row (s) / B col (n) within tile
    const int akcol = lane >> 4;         // k within the 4-wide micro-step
    const int NT = Npad >> 4;
    const int KQ = Mpad >> 2;            // k steps

    // every carve offset is a multiple of 16 B (the slice takes ds_write_b128)
    extern __shared__ __attribute__((aligned(16))) float lw_lds[];
    float* sums = lw_lds;                                // LW_S_TILE * NOUTP
    float* base_lds = sums + LW_S_TILE * NOUTP;          // NOUTP * 16
    float* slice = base_lds + NOUTP * 16;                // KQ*n_out*64

    // ---- A operand: one bit per (sub-tile, k step) and lane, 16 bits per
    // sub-tile (KQ <= 16), the four sub-tiles in one 64-bit register ---------
    // this thread's own cells of ``sums`` (rows akcol*4 + r of its wave's 16,
    // class arow) are zeroed here and touched by no other thread
    uint64_t abits = 0ull;
#pragma unroll
    for (int sub = 0; sub < LW_NSUB; ++sub) {
        const int srow = s0 + sub * LW_S_SUB + wave * 16 + arow;
        uint32_t bits = 0u;
        if (srow < S) {
            const uint8_t* mrow = masksU + ((size_t)b * S + srow) * M;
            for (int kq = 0; kq < KQ; ++kq) {
                const int k = kq * 4 + akcol;
                if (k < M) bits |= (uint32_t)(mrow[k] & 1) << kq;
            }
        }
        abits |= (uint64_t)bits << (16 * sub);
        if (arow < NOUTP) {
            const int sl = sub * LW_S_SUB + wave * 16 + akcol * 4;
#pragma unroll
            for (int r = 0; r < 4; ++r) sums[(sl + r) * NOUTP + arow] = 0.0f;
        }
    }

    const float* dsrc = diff + (size_t)b * NOUTP * Mpad * Npad;
    // per-lane B pointer: class and k step are added as immediates / one add
    const float* blane = slice + akcol * 16 + arow;
    const int kq_stride = n_out * 64;    // words per k step

#pragma unroll 1
    for (int ct = 0; ct < NT; ++ct) {
        __syncthreads();                 // every wave is done with the slice
        // ---- stage the column-tile slice [kq][o][k%4][16], real classes ----
        for (int idx = tid; idx < n_out * Mpad * 4; idx += LW_THREADS) {
            const int q = idx & 3;       // which float4 of the 16 columns
            const int ok = idx >> 2;
            const int o = ok / Mpad;
            const int k = ok - o * Mpad;
            const float4 v = *(const float4*)(
                dsrc + ((size_t)o * Mpad + k) * Npad + ct * 16 + q * 4);
            *(float4*)(slice + ((k >> 2) * n_out + o) * 64 + (k & 3) * 16
                       + q * 4) = v;
        }
        if (tid < n_out * 16)
            base_lds[tid] = base[(size_t)(tid >> 4) * Npad + ct * 16 + (tid & 15)];
        const float wn = wbg[ct * 16 + arow];
        __syncthreads();

        // (not unrolled: one copy of the k loop and the epilogue keeps the
        // register count at the accumulators' and the code in the I-cache)
#pragma unroll 1
        for (int sub = 0; sub < LW_NSUB; ++sub) {
            // wave-uniform: no barrier below, and the DPP reductions run with
            // all 64 lanes enabled
            if (s0 + sub * LW_S_SUB + wave * 16 >= S) break;
            const uint32_t bits = (uint32_t)(abits >> (16 * sub)) & 0xFFFFu;

            lw_f32x4 acc[NOUTP];
#pragma unroll
            for (int o = 0; o < NOUTP; ++o) acc[o] = (lw_f32x4){0, 0, 0, 0};

            const float* bp = blane;
#pragma unroll 1
            for (int kq = 0; kq < KQ; ++kq) {
                const float a = (float)((bits >> kq) & 1u);
#pragma unroll
                for (int o = 0; o < NOUTP; ++o) {
                    if (LW_REAL(o))
                        acc[o] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                            a, bp[o * 64], acc[o], 0, 0, 0);
                }
                bp += kq_stride;
            }

            // ---- epilogue, in place on the accumulators --------------------
            // C/D map: col n = lane&15, row s = (lane>>4)*4 + reg
#pragma unroll
            for (int o = 0; o < NOUTP; ++o) {
                if (LW_REAL(o)) {
                    const float bs = base_lds[o * 16 + arow];
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[o][r] += bs;
                }
            }
            float scale[4] = {wn, wn, wn, wn};
            if (ACT == 1) {
#pragma unroll
                for (int o = 0; o < NOUTP; ++o) {
                    if (LW_REAL(o)) {
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            acc[o][r] = lw_rcp(1.0f + __expf(-acc[o][r]));
                    }
                }
            } else if (ACT == 2) {
                // running maximum over the real classes only (class 0 is
                // always real), so exp never sees a positive argument
                float mx[4], sum[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) { mx[r] = acc[0][r]; sum[r] = 0.0f; }
#pragma unroll
                for (int o = 1; o < NOUTP; ++o) {
                    if (LW_REAL(o)) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) mx[r] = fmaxf(mx[r], acc[o][r]);
                    }
                }
#pragma unroll
                for (int o = 0; o < NOUTP; ++o) {
                    if (LW_REAL(o)) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            acc[o][r] = __expf(acc[o][r] - mx[r]);
                            sum[r] += acc[o][r];
                        }
                    }
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) scale[r] = wn * lw_rcp(sum[r]);
            }

            // weighted sum over the 16 columns; lane arow == o keeps class o
            float mine[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int o = 0; o < NOUTP; ++o) {
                if (LW_REAL(o)) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float v = lw_row16_sum(acc[o][r] * scale[r]);
                        mine[r] = (arow == o) ? v : mine[r];
                    }
                }
            }
            if (arow < n_out) {
                const int sl = sub * LW_S_SUB + wave * 16 + akcol * 4;
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    sums[(sl + r) * NOUTP + arow] += mine[r];
            }
        }  // sub-tile loop
    }  // column-tile loop

    // ---- write: the owner thread of each (s, o) cell stores it ------------
    if (arow < n_out) {
#pragma unroll
        for (int sub = 0; sub < LW_NSUB; ++sub) {
            const int sl = sub * LW_S_SUB + wave * 16 + akcol * 4;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ss = s0 + sl + r;
                if (ss < S)
                    ey[((size_t)b * S + ss) * n_out + arow] =
                        sums[(sl + r) * NOUTP + arow];
            }
        }
    }
}

template <int NOUTP>
static void launch_wide_act(
    const uint8_t* masksU, const float* diff, const float* base,
    const float* wbg, float* ey, int B, int S, int M, int Mpad, int Npad,
    int n_out, int act, hipStream_t stream)
{
    const int n_stiles = (S + LW_S_TILE - 1) / LW_S_TILE;
    dim3 grid(B * n_stiles), block(LW_THREADS);
    const size_t lds = (size_t)(LW_S_TILE * NOUTP + NOUTP * 16) * 4
                       + (size_t)n_out * Mpad * 16 * 4;
#define LW_CASE(ACTV) \
    case ACTV: \
        fused_predict_linear_wide_kernel<NOUTP, ACTV> \
            <<<grid, block, lds, stream>>>( \
                masksU, diff, base, wbg, ey, B, S, M, Mpad, Npad, n_out); \
        break;
    switch (act) { LW_CASE(0) LW_CASE(1) LW_CASE(2) }
#undef LW_CASE
}

// 0 on launch, -2 when the runtime rejects the launch (ey is then untouched),
// -1 outside the envelope: act in {0,1,2}; 3 <= n_out <= 16 with
// noutp the next multiple of 4; Mpad a multiple of 4 in [4, 64], M <= Mpad;
// Npad a multiple of 16 in [16, 512].
extern "C" int launch_fused_predict_linear_wide(
    const uint8_t* masksU, const float* diff, const float* base,
    const float* wbg, float* ey, int B, int S, int M, int Mpad, int Npad,
    int n_out, int noutp, int act, hipStream_t stream)
{
    if (act < 0 || act > 2) return -1;
    if (n_out < 3 || n_out > LW_MAX_NOUT || noutp != (n_out + 3) / 4 * 4)
        return -1;
    if (Mpad < 4 || Mpad > LW_MAX_MPAD || Mpad % 4 != 0 || M < 1 || M > Mpad)
        return -1;
    if (Npad < 16 || Npad > LW_MAX_NPAD || Npad % 16 != 0) return -1;
    if (B <= 0 || S <= 0) return 0;
    switch (noutp) {
        case 4: launch_wide_act<4>(masksU, diff, base, wbg, ey, B, S, M, Mpad, Npad, n_out, act, stream); break;
        case 8: launch_wide_act<8>(masksU, diff, base, wbg, ey, B, S, M, Mpad, Npad, n_out, act, stream); break;
        case 12: launch_wide_act<12>(masksU, diff, base, wbg, ey, B, S, M, Mpad, Npad, n_out, act, stream); break;
        default: launch_wide_act<16>(masksU, diff, base, wbg, ey, B, S, M, Mpad, Npad, n_out, act, stream); break;
    }
    // the dynamic LDS request reaches 99,328 B: a rejected launch must not
    // pass for a result
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
