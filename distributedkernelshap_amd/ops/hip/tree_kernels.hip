// MI355X (gfx950) fused predict kernel for tree-ensemble predictors.
//
//   K4t fused_predict_trees — per instance b, coalition sample s and
//       background row n, the perturbation row is
//           row[j] = mask[b,s,g(j)] ? x[b,j] : bg[n,j]
//       and the decision at an internal node i of tree t is
//           mask[b,s,g(feat_i)] ? (x[b,feat_i] <= thr_i) : (bg[n,feat_i] <= thr_i).
//       Both comparisons are independent of s: they arrive packed to bits,
//       dx (B,T) and dbg (N,T), one u64 per tree (<= 64 internal nodes).  With
//           nm[t]  = OR of the node masks of tree t's groups that are ON in s
//           c      = dbg[n,t] ^ ((dx[b,t] ^ dbg[n,t]) & nm[t])
//       the walk is node = child[t][node][(c >> node) & 1] until a leaf code
//       (>= 64) appears.  raw[o] = base[o] + scale * sum_t leaf, then the
//       output activation, then ey[b,s,:] = sum_n wbg[n] * p.
//       No feature value, threshold or perturbation row is touched here, and
//       only ey reaches global memory.
//
// Decomposition: one 1024-thread workgroup (16 waves) owns (b, SP consecutive
// samples), SP = 64, 32 or 16.  The build phase computes nm[t][sample] for
// every tree once into LDS (8 B x SP per tree) and stages the child table
// (2 B per internal node) and, when they fit, the leaf values; all three are
// then reused for every background row.  In the main loop a lane owns one
// sample and one of NW * 64 / SP "n slots"; slot k visits n = k, k + slots,
// ...  With SP = 64 the slot is the wave, so dx[b,t], dbg[n,t] and the tree
// header are wave-uniform (scalar) loads.  Each lane accumulates wbg[n] * p in
// registers; the slots are combined through LDS in slot order — no float
// atomics, no partials in global memory, bitwise deterministic.  SP shrinks
// only so that nm fits the 160 KiB of LDS when there are many trees; the
// launcher picks the largest SP that leaves room for two workgroups per CU
// (more resident waves hide the dependent LDS reads of the walk), else the
// largest that fits at all.
//
// This is integer and LDS work; there is nothing for the matrix cores here.

#include <hip/hip_runtime.h>
#include <cstdint>
#include <mutex>

#define TR_MAX_DEVICES 64
#define TR_THREADS 1024         // 16 waves: the walk is latency-bound
#define TR_MAX_NOUT 8
#define TR_MAX_NODES 64          // internal nodes per tree (one u64 of decisions)
#define TR_MAX_TREES 1024
#define TR_LDS_BYTES (160 * 1024)

struct TreeArgs {
    const uint8_t* masks;        // (B, S, Mv) u8
    const int* vmap;             // (G) group -> varying index, -1 = not varying
    const uint64_t* dx;          // (B, T)
    const uint64_t* dbg;         // (N, T)
    const uint8_t* child;        // (C, 2) u8, C a multiple of 8
    const int4* meta;            // (T) {child offset, leaf offset, out col, I}
    const float* leaves;         // (L) or (L, n_out)
    const int* grp_off;          // (T + 1)
    const int* grp_id;           // (E)
    const uint64_t* grp_mask;    // (E)
    const float* base;           // (n_out)
    const float* wbg;            // (N)
    float* ey;                   // (B, S, n_out)
    float scale;
    int B, S, Mv, N, T, G, E, L, n_out, act, leaf_mode;
    int leaves_in_lds;
    unsigned nm_bytes, child_bytes, leaf_bytes;
};

template <int SP, int NO>
__global__ __launch_bounds__(TR_THREADS)
void fused_predict_trees_kernel(const TreeArgs p)
{
    extern __shared__ __align__(16) unsigned char tr_smem[];
    uint64_t* nm = reinterpret_cast<uint64_t*>(tr_smem);            // [T][SP]
    uint8_t* childL = tr_smem + p.nm_bytes;                         // [C][2]
    float* leafL = reinterpret_cast<float*>(tr_smem + p.nm_bytes + p.child_bytes);

    constexpr int SUB = 64 / SP;          // n slots per wave
    const int tid = threadIdx.x;
    const int nthreads = blockDim.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int nslots = (nthreads >> 6) * SUB;
    const int n_tiles = (p.S + SP - 1) / SP;
    const int b = blockIdx.x / n_tiles;
    const int s0 = (blockIdx.x % n_tiles) * SP;
    const int T = p.T;

    // ---- build phase: child table, leaves, nm[t][sample] -> LDS ----------
    {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(p.child);
        uint32_t* dst = reinterpret_cast<uint32_t*>(childL);
        for (int i = tid; i < (int)(p.child_bytes >> 2); i += nthreads) dst[i] = src[i];
    }
    if (p.leaves_in_lds) {
        for (int i = tid; i < (int)(p.leaf_bytes >> 2); i += nthreads)
            leafL[i] = p.leaves[i];
    }
    for (int i = tid; i < T * SP; i += nthreads) {
        const int t = i / SP;
        const int sl = i % SP;
        const int s = min(s0 + sl, p.S - 1);     // tail lanes repeat the last row
        const uint8_t* mrow = p.masks + ((size_t)b * p.S + s) * p.Mv;
        const int e1 = min(p.grp_off[t + 1], p.E);
        uint64_t m = 0;
        for (int e = p.grp_off[t]; e < e1; ++e) {
            const int g = p.grp_id[e];
            const int vi = (g >= 0 && g < p.G) ? p.vmap[g] : -1;
            // a group that does not vary keeps the background's decisions
            if (vi >= 0 && vi < p.Mv && mrow[vi]) m |= p.grp_mask[e];
        }
        nm[i] = m;
    }
    __syncthreads();

    // ---- main loop: lane = (sample, n slot) -------------------------------
    const int sl = lane % SP;
    int slot = wave * SUB + lane / SP;
    if (SP == 64) slot = __builtin_amdgcn_readfirstlane(slot);   // wave-uniform n

    float acc[NO];
#pragma unroll
    for (int o = 0; o < NO; ++o) acc[o] = 0.0f;

    const uint64_t* dxb = p.dx + (size_t)b * T;
    const int lstride = p.leaf_mode ? p.n_out : 1;
    for (int n = slot; n < p.N; n += nslots) {
        const uint64_t* dbn = p.dbg + (size_t)n * T;
        float raw[NO];
#pragma unroll
        for (int o = 0; o < NO; ++o) raw[o] = 0.0f;

        for (int t = 0; t < T; ++t) {
            const int4 mt = p.meta[t];
            const uint64_t g = dbn[t];
            const uint64_t c = g ^ ((dxb[t] ^ g) & nm[t * SP + sl]);
            const uint8_t* ch = childL + 2 * mt.x;
            unsigned node = 0;
            // a well-formed table ends within 64 steps; the bound keeps a
            // malformed one from spinning
            for (int step = 0; step < TR_MAX_NODES && node < TR_MAX_NODES; ++step)
                node = ch[2 * node + (unsigned)((c >> node) & 1ull)];
            const int leaf = node >= TR_MAX_NODES ? (int)node - TR_MAX_NODES : 0;
            const int li = min(mt.y + leaf, p.L - 1) * lstride;
            if (p.leaf_mode == 0) {
                const float v = p.leaves_in_lds ? leafL[li] : p.leaves[li];
#pragma unroll
                for (int o = 0; o < NO; ++o)
                    if (o == mt.z) raw[o] += v;
            } else {
#pragma unroll
                for (int o = 0; o < NO; ++o)
                    if (o < p.n_out)
                        raw[o] += p.leaves_in_lds ? leafL[li + o] : p.leaves[li + o];
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

    // ---- combine the n slots in slot order (red overlays nm) -------------
    __syncthreads();
    float* red = reinterpret_cast<float*>(tr_smem);      // [slot][SP][NO]
#pragma unroll
    for (int o = 0; o < NO; ++o)
        red[((size_t)(wave * SUB + lane / SP) * SP + sl) * NO + o] = acc[o];
    __syncthreads();
    for (int i = tid; i < SP * NO; i += nthreads) {
        const int rs = i / NO;
        const int o = i % NO;
        float sum = 0.0f;
        for (int k = 0; k < nslots; ++k) sum += red[((size_t)k * SP + rs) * NO + o];
        const int s = s0 + rs;
        if (s < p.S && o < p.n_out)
            p.ey[((size_t)b * p.S + s) * p.n_out + o] = sum;
    }
}

static unsigned tr_round16(size_t v) { return (unsigned)((v + 15) / 16 * 16); }

template <int SP, int NO>
static int launch_trees_t(TreeArgs& a, size_t lds, hipStream_t stream)
{
    if (lds > 48 * 1024) {
        // the attribute is per function and device and only ever needs to
        // grow: remember the size already granted and skip the call below it
        static std::mutex mtx;
        static size_t granted[TR_MAX_DEVICES] = {};
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) return -2;
        const bool cached = dev >= 0 && dev < TR_MAX_DEVICES;
        std::lock_guard<std::mutex> lock(mtx);
        if (!cached || granted[dev] < lds) {
            if (hipFuncSetAttribute(
                    reinterpret_cast<const void*>(&fused_predict_trees_kernel<SP, NO>),
                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)
                != hipSuccess)
                return -2;
            if (cached) granted[dev] = lds;
        }
    }
    const long long n_tiles = (a.S + SP - 1) / SP;
    const long long nblk = (long long)a.B * n_tiles;
    if (nblk > 0x7fffffffLL) return -1;
    dim3 grid((unsigned)nblk), block(TR_THREADS);
    fused_predict_trees_kernel<SP, NO><<<grid, block, lds, stream>>>(a);
    return 0;
}

template <int NO>
static int launch_trees_sp(TreeArgs& a, int sp, size_t lds, hipStream_t stream)
{
    if (sp == 64) return launch_trees_t<64, NO>(a, lds, stream);
    if (sp == 32) return launch_trees_t<32, NO>(a, lds, stream);
    return launch_trees_t<16, NO>(a, lds, stream);
}

// Returns -1 outside the supported envelope: 1..1024 trees of at most 64
// internal nodes, n_out <= 8, and nm at 16 samples per workgroup (128 B per
// tree) plus the child table (2 B per internal node) within 160 KiB of LDS.
// Any B, S, N, D and any number of varying groups.
extern "C" int launch_fused_predict_trees(
    const uint8_t* masks, const int* vmap, const int64_t* dx, const int64_t* dbg,
    const uint8_t* child, const int* meta, const float* leaves,
    const int* grp_off, const int* grp_id, const int64_t* grp_mask,
    const float* base, const float* wbg, float* ey, float scale,
    int B, int S, int Mv, int N, int T, int G, int E, int L, int C,
    int max_internal, int n_out, int act, int leaf_mode, hipStream_t stream)
{
    if (B < 1 || S < 1 || N < 1 || Mv < 1 || G < 1 || L < 1 || C < 1) return -1;
    if (T < 1 || T > TR_MAX_TREES) return -1;
    if (max_internal < 1 || max_internal > TR_MAX_NODES) return -1;
    if (n_out < 1 || n_out > TR_MAX_NOUT) return -1;
    if (act < 0 || act > 2 || leaf_mode < 0 || leaf_mode > 1) return -1;
    if (C % 8 != 0) return -1;

    const int no = n_out <= 1 ? 1 : n_out <= 2 ? 2 : n_out <= 4 ? 4 : 8;
    const size_t red_bytes = (size_t)TR_THREADS * no * sizeof(float);
    const size_t child_bytes = (size_t)C * 2;
    const size_t leaf_bytes =
        tr_round16((size_t)L * (leaf_mode ? n_out : 1) * sizeof(float));
    int sp = 0;
    size_t nm_bytes = 0;
    const size_t limits[2] = {TR_LDS_BYTES / 2, TR_LDS_BYTES};
    for (int pass = 0; pass < 2 && sp == 0; ++pass) {
        for (int cand = 64; cand >= 16; cand >>= 1) {
            size_t nmb = (size_t)T * cand * sizeof(uint64_t);
            if (nmb < red_bytes) nmb = red_bytes;
            nmb = tr_round16(nmb);
            if (nmb + child_bytes <= limits[pass]) {
                sp = cand; nm_bytes = nmb;
                break;
            }
        }
    }
    if (sp == 0) return -1;
    size_t lds = nm_bytes + child_bytes;
    const size_t cap = lds <= TR_LDS_BYTES / 2 ? TR_LDS_BYTES / 2 : TR_LDS_BYTES;
    const int leaves_in_lds = lds + leaf_bytes <= cap;
    if (leaves_in_lds) lds += leaf_bytes;

    TreeArgs a;
    a.masks = masks; a.vmap = vmap;
    a.dx = reinterpret_cast<const uint64_t*>(dx);
    a.dbg = reinterpret_cast<const uint64_t*>(dbg);
    a.child = child; a.meta = reinterpret_cast<const int4*>(meta);
    a.leaves = leaves; a.grp_off = grp_off; a.grp_id = grp_id;
    a.grp_mask = reinterpret_cast<const uint64_t*>(grp_mask);
    a.base = base; a.wbg = wbg; a.ey = ey; a.scale = scale;
    a.B = B; a.S = S; a.Mv = Mv; a.N = N; a.T = T; a.G = G; a.E = E; a.L = L;
    a.n_out = n_out; a.act = act; a.leaf_mode = leaf_mode;
    a.leaves_in_lds = leaves_in_lds;
    a.nm_bytes = (unsigned)nm_bytes; a.child_bytes = (unsigned)child_bytes;
    a.leaf_bytes = (unsigned)((size_t)L * (leaf_mode ? n_out : 1) * sizeof(float));

    switch (no) {
    case 1: return launch_trees_sp<1>(a, sp, lds, stream);
    case 2: return launch_trees_sp<2>(a, sp, lds, stream);
    case 4: return launch_trees_sp<4>(a, sp, lds, stream);
    default: return launch_trees_sp<8>(a, sp, lds, stream);
    }
}
