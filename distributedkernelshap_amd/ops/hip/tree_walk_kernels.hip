// MI355X (gfx950) fused predict kernel for deep tree ensembles.
//
//   K4w fused_predict_trees_walk — for trees beyond the 64 internal nodes
//       that fused_predict_trees (tree_kernels.hip) keeps in one u64.  Per
//       instance b, coalition sample s, background row n and tree t the tree
//       is walked on the blended row
//           row[j] = mask[b,s,g(j)] ? x[b,j] : bg[n,j]
//       without building that row:
//           rec  = nodes[node]                       one 16-byte record
//           on   = groupbits[s] has bit rec.group
//           v    = on ? x[b, rec.feature] : bg[n, rec.feature]
//           node = (v <= rec.thr32) ? node + 1 : rec.right
//       until a leaf record (feature < 0) appears.  raw[o] = base[o] + scale *
//       sum_t leaf, then the output activation, then
//       ey[b,s,:] = sum_n wbg[n] * p.  Only ey reaches global memory.
//
// Node table (built once by ops/tree_pack.py: pack_trees_walk): the nodes of a
// tree are numbered in preorder, so the left child is node + 1 and a record
// stores only the right child.  int4 {thr32 bits, feature, group, right} for a
// split, {value bits, -1, out column, leaf row} for a leaf (a scalar leaf
// carries its float32 value, which saves the walk's last dependent load; a
// vector leaf's row is read from the leaf table).  thr32 is the largest
// float32 not above the float64 threshold, so the float32 compare equals
// sklearn's "round the input to float32, compare in float64".  The table is
// read through L1/L2 (a default random forest is about 1.25 MB).
//
// Decomposition (as fused_predict_trees): one 1024-thread workgroup owns
// (b, 64 consecutive samples); a lane is a sample and a wave is an n slot, so
// the background row is wave-uniform.  The build phase stages x[b,:], the
// per-sample bitset of switched-on groups (one u64 per 64 groups) and, when
// it fits beside them in half of the LDS, the whole background.  Each lane
// accumulates wbg[n] * p in registers; the slots are combined through LDS in
// slot order — no float atomics, no partials in global memory, bitwise
// deterministic.  Two trees are walked per lane at a time so that their
// record loads overlap (measured: 1.48x one tree at a time; four gain 1.5 %
// more).
//
// Routed tables (ROUTED = true; RoutedTreeEnsemblePredictor): x and bg hold
// encoded rows (a feature with known categories is its category index or
// NaN) and a split record carries two flags above the group in [2]:
//     bit 30  a missing value goes left
//     bit 29  categorical split; [0] is then a row of cat_left (C, 8) u32,
//             a bitset of 256 bits, bit c set = "code c goes left"
// The step becomes
//     numeric      left = (v != v) ? missing_left : v <= thr32
//     categorical  missing = !(0 <= v < 256)          (true for NaN)
//                  c = (int)v
//                  left = missing ? missing_left
//                                 : bit c of cat_left[row * 8 + (c >> 5)]
// with one dependent dword load for a categorical split only.  The ROUTED =
// false instantiations are the code they were before the flag existed.
//
// Every index taken from a record is clamped before it is used (the bitset
// row to C - 1; the launcher refuses C < 1), and a walk ends after 64 steps:
// a malformed table gives wrong numbers, never a read out of bounds or a
// spin.

#include <hip/hip_runtime.h>
#include <cstdint>
#include <mutex>

#define TW_MAX_DEVICES 64
#define TW_THREADS 1024          // 16 waves: the walk is latency-bound
#define TW_MAX_NOUT 8
#define TW_MAX_DEPTH 64          // step bound of one walk
#define TW_MAX_GROUPS 1024       // 16 u64 words per sample in LDS
#define TW_MAX_FEATURES 4096     // x row of 16 KiB in LDS
#define TW_LDS_HALF (80 * 1024)  // two workgroups per CU
#define TW_IL 2                  // trees walked per lane at a time
#define TW_GROUP_MASK 0xffff     // routed record [2]: group in the low bits,
#define TW_FLAG_MISSING_LEFT (1 << 30)   // then the two routing flags
#define TW_FLAG_CATEGORICAL (1 << 29)
#define TW_CAT_WORDS 8           // 256 bits per categorical split

struct WalkArgs {
    const uint8_t* masks;        // (B, S, Mv) u8
    const int* vmap;             // (G) group -> varying index, -1 = not varying
    const float* x;              // (B, D)
    const float* bg;             // (N, D)
    const int4* nodes;           // (R) records
    const int* roots;            // (T) record index of each tree's root
    const float* leaves;         // (L) or (L, n_out)
    const float* base;           // (n_out)
    const float* wbg;            // (N)
    float* ey;                   // (B, S, n_out)
    float scale;
    int B, S, Mv, N, D, G, T, R, L, n_out, act, leaf_mode;
    int gwords;                  // ceil(G / 64)
    unsigned x_bytes, gb_bytes;
    const unsigned* cat_left;    // (C, 8) u32 bitsets, routed tables only
    int C;
};

template <int NO, bool WIDE, bool BGL, bool ROUTED>
__global__ __launch_bounds__(TW_THREADS)
void fused_predict_trees_walk_kernel(const WalkArgs p)
{
    extern __shared__ __align__(16) unsigned char tw_smem[];
    float* xL = reinterpret_cast<float*>(tw_smem);                        // [D]
    uint64_t* gbL = reinterpret_cast<uint64_t*>(tw_smem + p.x_bytes);     // [W][64]
    float* bgL = reinterpret_cast<float*>(tw_smem + p.x_bytes + p.gb_bytes);

    const int tid = threadIdx.x;
    const int nthreads = blockDim.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nwaves = nthreads >> 6;
    const int n_tiles = (p.S + 63) / 64;
    const int b = blockIdx.x / n_tiles;
    const int s0 = (blockIdx.x % n_tiles) * 64;
    const int D = p.D;
    constexpr int IL = TW_IL;

    // ---- build phase: x row, group bitsets, background -> LDS ------------
    for (int i = tid; i < D; i += nthreads) xL[i] = p.x[(size_t)b * D + i];
    if (BGL) {
        for (int i = tid; i < p.N * D; i += nthreads) bgL[i] = p.bg[i];
    }
    for (int i = tid; i < p.gwords * 64; i += nthreads) {
        const int w = i >> 6;
        const int s = min(s0 + (i & 63), p.S - 1);   // tail lanes repeat the last row
        const uint8_t* mrow = p.masks + ((size_t)b * p.S + s) * p.Mv;
        const int g1 = min(p.G, (w + 1) * 64);
        uint64_t m = 0;
        for (int g = w * 64; g < g1; ++g) {
            const int vi = p.vmap[g];
            // a group that does not vary keeps the background's value
            if (vi >= 0 && vi < p.Mv && mrow[vi]) m |= 1ull << (g & 63);
        }
        gbL[i] = m;
    }
    __syncthreads();

    // ---- main loop: lane = sample, wave = n slot --------------------------
    const uint64_t gb0 = gbL[lane];
    const unsigned rmax = (unsigned)p.R - 1u;
    const unsigned cmax = ROUTED ? (unsigned)p.C - 1u : 0u;
    const int lstride = p.leaf_mode ? p.n_out : 1;

    float acc[NO];
#pragma unroll
    for (int o = 0; o < NO; ++o) acc[o] = 0.0f;

    for (int n = wave; n < p.N; n += nwaves) {
        const float* bgrow = BGL ? bgL + n * D : p.bg + (size_t)n * D;
        float raw[NO];
#pragma unroll
        for (int o = 0; o < NO; ++o) raw[o] = 0.0f;

        for (int t = 0; t < p.T; t += IL) {
            unsigned node[IL];
            int4 rec[IL];
#pragma unroll
            for (int k = 0; k < IL; ++k) {
                node[k] = min((unsigned)p.roots[min(t + k, p.T - 1)], rmax);
                rec[k] = p.nodes[node[k]];
                if (t + k >= p.T) { rec[k].y = -1; rec[k].w = -1; }   // no tree
            }
            // a well-formed table ends within 64 steps; the bound keeps a
            // malformed one from spinning
            for (int step = 0; step < TW_MAX_DEPTH; ++step) {
                bool any = false;
#pragma unroll
                for (int k = 0; k < IL; ++k) any |= rec[k].y >= 0;
                if (!any) break;
#pragma unroll
                for (int k = 0; k < IL; ++k) {
                    if (rec[k].y >= 0) {
                        const int f = min(rec[k].y, D - 1);
                        const int g = ROUTED ? (rec[k].z & TW_GROUP_MASK)
                                             : rec[k].z;
                        const uint64_t word = WIDE
                            ? gbL[min((int)((unsigned)g >> 6), p.gwords - 1) * 64 + lane]
                            : gb0;
                        const float vx = xL[f];
                        const float vb = bgrow[f];
                        const float v = ((word >> (g & 63)) & 1ull) ? vx : vb;
                        // a NaN compare is false and must not decide: the
                        // explicit test sends a missing value by its flag.
                        // Bitwise, not short-circuit: the numeric step stays
                        // straight-line code (the loop is bound by the
                        // instructions it issues, see docs/DESIGN.md)
                        bool left = v <= __int_as_float(rec[k].x);
                        if (ROUTED) {
                            const bool ml = (rec[k].z & TW_FLAG_MISSING_LEFT) != 0;
                            left = left | ((v != v) & ml);
                            if (rec[k].z & TW_FLAG_CATEGORICAL) {
                                // NaN fails both compares: the range test
                                // comes before the float -> int conversion
                                const bool known = v >= 0.0f && v < 256.0f;
                                const int c = known ? (int)v : 0;
                                const unsigned row = min((unsigned)rec[k].x, cmax);
                                const unsigned w =
                                    p.cat_left[row * TW_CAT_WORDS + (c >> 5)];
                                left = known ? ((w >> (c & 31)) & 1u) != 0 : ml;
                            }
                        }
                        const unsigned nx = left ? node[k] + 1u
                                                 : (unsigned)rec[k].w;
                        node[k] = min(nx, rmax);
                        rec[k] = p.nodes[node[k]];
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < IL; ++k) {
                if (rec[k].y < 0 && rec[k].w >= 0) {
                    if (p.leaf_mode == 0) {
                        // a scalar leaf carries its value: no further load
                        const float v = __int_as_float(rec[k].x);
#pragma unroll
                        for (int o = 0; o < NO; ++o)
                            if (o == rec[k].z) raw[o] += v;
                    } else {
                        const int li = min(rec[k].w, p.L - 1) * lstride;
#pragma unroll
                        for (int o = 0; o < NO; ++o)
                            if (o < p.n_out) raw[o] += p.leaves[li + o];
                    }
                }
            }
        }

        float z[NO];
#pragma unroll
        for (int o = 0; o < NO; ++o)
            z[o] = o < p.n_out ? p.base[o] + p.scale * raw[o] : 0.0f;
        const float wn = p.wbg[n];
        if (p.act == 2) {
            float mx = z[0];
#pragma unroll
            for (int o = 1; o < NO; ++o)
                if (o < p.n_out) mx = fmaxf(mx, z[o]);
            float sum = 0.0f;
#pragma unroll
            for (int o = 0; o < NO; ++o) {
                z[o] = o < p.n_out ? __expf(z[o] - mx) : 0.0f;
                sum += z[o];
            }
            const float inv = 1.0f / sum;
#pragma unroll
            for (int o = 0; o < NO; ++o) acc[o] += wn * (z[o] * inv);
        } else if (p.act == 1) {
#pragma unroll
            for (int o = 0; o < NO; ++o)
                acc[o] += wn * (1.0f / (1.0f + __expf(-z[o])));
        } else {
#pragma unroll
            for (int o = 0; o < NO; ++o) acc[o] += wn * z[o];
        }
    }

    // ---- combine the n slots in slot order (red overlays the staging) -----
    __syncthreads();
    float* red = reinterpret_cast<float*>(tw_smem);      // [slot][64][NO]
#pragma unroll
    for (int o = 0; o < NO; ++o)
        red[((size_t)wave * 64 + lane) * NO + o] = acc[o];
    __syncthreads();
    for (int i = tid; i < 64 * NO; i += nthreads) {
        const int rs = i / NO;
        const int o = i % NO;
        float sum = 0.0f;
        for (int k = 0; k < nwaves; ++k) sum += red[((size_t)k * 64 + rs) * NO + o];
        const int s = s0 + rs;
        if (s < p.S && o < p.n_out)
            p.ey[((size_t)b * p.S + s) * p.n_out + o] = sum;
    }
}

static size_t tw_round16(size_t v) { return (v + 15) / 16 * 16; }

template <int NO, bool WIDE, bool BGL, bool ROUTED>
static int launch_walk_t(WalkArgs& a, size_t lds, hipStream_t stream)
{
    if (lds > 48 * 1024) {
        // the attribute is per function and device and only ever needs to
        // grow: remember the size already granted and skip the call below it
        static std::mutex mtx;
        static size_t granted[TW_MAX_DEVICES] = {};
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) return -2;
        const bool cached = dev >= 0 && dev < TW_MAX_DEVICES;
        std::lock_guard<std::mutex> lock(mtx);
        if (!cached || granted[dev] < lds) {
            if (hipFuncSetAttribute(
                    reinterpret_cast<const void*>(
                        &fused_predict_trees_walk_kernel<NO, WIDE, BGL, ROUTED>),
                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)
                != hipSuccess)
                return -2;
            if (cached) granted[dev] = lds;
        }
    }
    const long long n_tiles = (a.S + 63) / 64;
    const long long nblk = (long long)a.B * n_tiles;
    if (nblk > 0x7fffffffLL) return -1;
    dim3 grid((unsigned)nblk), block(TW_THREADS);
    fused_predict_trees_walk_kernel<NO, WIDE, BGL, ROUTED>
        <<<grid, block, lds, stream>>>(a);
    return 0;
}

template <int NO, bool ROUTED>
static int launch_walk_r(WalkArgs& a, bool wide, bool bgl, size_t lds,
                         hipStream_t stream)
{
    if (wide)
        return bgl ? launch_walk_t<NO, true, true, ROUTED>(a, lds, stream)
                   : launch_walk_t<NO, true, false, ROUTED>(a, lds, stream);
    return bgl ? launch_walk_t<NO, false, true, ROUTED>(a, lds, stream)
               : launch_walk_t<NO, false, false, ROUTED>(a, lds, stream);
}

template <int NO>
static int launch_walk_no(WalkArgs& a, bool wide, bool bgl, size_t lds,
                          hipStream_t stream)
{
    return a.cat_left ? launch_walk_r<NO, true>(a, wide, bgl, lds, stream)
                      : launch_walk_r<NO, false>(a, wide, bgl, lds, stream);
}

// Returns -1 outside the supported envelope: any number of trees and records
// that int32 holds, depth <= 64, n_out <= 8, G <= 1024 groups, D <= 4096
// features.  Any B, S, N and any number of varying groups.  LDS per
// workgroup: 4 B x D (x row) + 512 B x ceil(G / 64) (group bitsets) + 4 B x
// N x D (background, only while the three stay within 80 KiB), at least the
// reduction scratch of 4 KiB x n_out rounded up to 1, 2, 4 or 8.
// cat_left = nullptr (with C = 0) walks plain tables; a routed table passes
// its C >= 1 bitset rows, and x and bg hold encoded rows.
extern "C" int launch_fused_predict_trees_walk(
    const uint8_t* masks, const int* vmap, const float* x, const float* bg,
    const int* nodes, const int* roots, const float* leaves, const float* base,
    const float* wbg, float* ey, float scale,
    int B, int S, int Mv, int N, int D, int G, int T, int R, int L,
    int max_depth, int n_out, int act, int leaf_mode,
    const unsigned* cat_left, int C, hipStream_t stream)
{
    if (cat_left ? (C < 1 || C > 0x7fffffff / TW_CAT_WORDS) : C != 0) return -1;
    if (B < 1 || S < 1 || N < 1 || Mv < 1 || L < 1 || T < 1 || R < 1) return -1;
    if (D < 1 || D > TW_MAX_FEATURES) return -1;
    if (G < 1 || G > TW_MAX_GROUPS) return -1;
    if (max_depth < 0 || max_depth > TW_MAX_DEPTH) return -1;
    if (n_out < 1 || n_out > TW_MAX_NOUT) return -1;
    if (act < 0 || act > 2 || leaf_mode < 0 || leaf_mode > 1) return -1;

    const int no = n_out <= 1 ? 1 : n_out <= 2 ? 2 : n_out <= 4 ? 4 : 8;
    const int gwords = (G + 63) / 64;
    const size_t red_bytes = (size_t)TW_THREADS * no * sizeof(float);
    const size_t x_bytes = tw_round16((size_t)D * sizeof(float));
    const size_t gb_bytes = (size_t)gwords * 64 * sizeof(uint64_t);
    const size_t bg_bytes = (size_t)N * D * sizeof(float);
    const bool bgl = x_bytes + gb_bytes + bg_bytes <= TW_LDS_HALF;
    size_t lds = x_bytes + gb_bytes + (bgl ? bg_bytes : 0);
    if (lds < red_bytes) lds = red_bytes;

    WalkArgs a;
    a.masks = masks; a.vmap = vmap; a.x = x; a.bg = bg;
    a.nodes = reinterpret_cast<const int4*>(nodes); a.roots = roots;
    a.leaves = leaves; a.base = base; a.wbg = wbg; a.ey = ey; a.scale = scale;
    a.B = B; a.S = S; a.Mv = Mv; a.N = N; a.D = D; a.G = G; a.T = T; a.R = R;
    a.L = L; a.n_out = n_out; a.act = act; a.leaf_mode = leaf_mode;
    a.gwords = gwords;
    a.x_bytes = (unsigned)x_bytes; a.gb_bytes = (unsigned)gb_bytes;
    a.cat_left = cat_left; a.C = C;

    const bool wide = gwords > 1;
    switch (no) {
    case 1: return launch_walk_no<1>(a, wide, bgl, lds, stream);
    case 2: return launch_walk_no<2>(a, wide, bgl, lds, stream);
    case 4: return launch_walk_no<4>(a, wide, bgl, lds, stream);
    default: return launch_walk_no<8>(a, wide, bgl, lds, stream);
    }
}
