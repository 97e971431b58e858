// Torch bindings for the CDNA4 KernelSHAP kernels (kshap_kernels.hip,
// linear_wide_kernels.hip, mlp_kernels.hip, tree_kernels.hip, km_kernels.hip).
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <c10/hip/HIPStream.h>

#include <cstdint>

extern "C" void launch_fill_random_masks(
    uint8_t* masks, int B, int S, int M, int ne, int n_random,
    const float* cdf, const int* sizes, int n_sizes, int num_paired,
    uint32_t seed, const int32_t* inst_ids, hipStream_t stream);

extern "C" int launch_fused_predict_linear(
    const uint8_t* masksU, const float* diff, const float* base, const float* wbg,
    float* ey, int B, int S, int M, int Mpad, int Npad, int n_out, int act,
    hipStream_t stream);

// linear_wide_kernels.hip
extern "C" int launch_fused_predict_linear_wide(
    const uint8_t* masksU, const float* diff, const float* base,
    const float* wbg, float* ey, int B, int S, int M, int Mpad, int Npad,
    int n_out, int noutp, int act, hipStream_t stream);

extern "C" void launch_synth_chunk(
    const uint8_t* masks, const float* x, const float* bg, const int* col_group,
    void* out, int out_bf16, int S, int M, int N, int D, int b_lo, int b_hi,
    int s_lo, int s_hi, hipStream_t stream);

// bf16 device pointers are opaque 16-bit words host-side (extern "C")
extern "C" void launch_pack_masks(
    const uint8_t* masks, uint64_t* packed, int B, int S, int M,
    hipStream_t stream);

extern "C" int launch_fused_predict_bf16(
    const uint8_t* masksU, const uint16_t* diffB,
    const float* base, const float* wbg, float* ey, int B, int S, int M,
    int Npad, int n_out, int act, int split, hipStream_t stream);

extern "C" void launch_build_diff_f32(
    const float* xp, const float* bgp, const int64_t* vidx, float* out,
    int B, int G, int O, int N, int m, int Mpad, int Npad, hipStream_t stream);

extern "C" void launch_build_diff_bf16(
    const float* xp, const float* bgp, const int64_t* vidx, uint16_t* out,
    int B, int G, int O, int N, int m, int Npad, int split, hipStream_t stream);

extern "C" int launch_wls_solve(
    const uint8_t* masks, const uint64_t* packed, const float* kw,
    const float* ey_adj, const float* total, float* phi, int B, int S, int M,
    int n_out, hipStream_t stream);

extern "C" void launch_pack_masks_words(
    const uint8_t* masks, uint64_t* packed, int B, int S, int M, int W,
    hipStream_t stream);

extern "C" int launch_wls_gram(
    const uint64_t* packed, const float* kw, const float* ey_adj,
    const float* total, double* A64, double* rhs64, int B, int S, int M,
    int W, int n_out, hipStream_t stream);

extern "C" int launch_fused_predict_tiled(
    const uint8_t* masksU, const float* diff, const float* base,
    const float* wbg, float* partial, float* ey, int B, int S, int M,
    int Mpad, int Npad, int n_out, int act, hipStream_t stream);

extern "C" void launch_build_diff_bf16_tiled(
    const float* xp, const float* bgp, const int64_t* vidx, uint16_t* out,
    int B, int G, int O, int N, int m, int Mpad, int Npad, int split,
    hipStream_t stream);

extern "C" int launch_fused_predict_tiled_bf16(
    const uint8_t* masksU, const uint16_t* diffB, const float* base,
    const float* wbg, float* partial, float* ey, int B, int S, int M,
    int Mpad, int Npad, int n_out, int act, int split, hipStream_t stream);

// packed linear pipeline
extern "C" int launch_fill_masks_packed(
    uint64_t* packed, const uint64_t* enum_packed, int B, int S, int M, int ne,
    int n_random, const float* cdf, const int* sizes, int n_sizes,
    int num_paired, uint32_t seed, const int32_t* inst_ids, hipStream_t stream);

extern "C" int launch_linear_prepare(
    const float* X, const float* W, const float* bias,
    const int64_t* col_group, const int64_t* vidx, const float* bgp,
    const double* lfnull64, float* diff, float* total, int B, int D, int G,
    int N, int m, int Mpad, int Npad, int n_out, int act, int link,
    hipStream_t stream);

extern "C" int launch_fused_predict_linear_packed(
    const uint64_t* packed, const float* diff, const float* base,
    const float* wbg, const float* lfnull, float* ey, int B, int S, int Mpad,
    int Npad, int n_out, int act, int link, hipStream_t stream, int mma);

extern "C" int launch_wls_solve_packed(
    const uint64_t* packed, const float* kw, const float* ey_adj,
    const float* total, const int64_t* vidx, float* phi_full, int B, int S,
    int M, int n_out, int G, hipStream_t stream);

extern "C" int launch_varying_probe(
    const float* X, const float* bg_min, const float* bg_max,
    const float* tol_min, const float* tol_max, const int64_t* col_group,
    int64_t* keys, int64_t* probe, int B, int D, int G, hipStream_t stream);

// mlp_kernels.hip
extern "C" int launch_fused_predict_mlp(
    const uint8_t* masks, const void* xp1, const void* bgp1n,
    const float* base1, const void* const* hw, const float* const* hb,
    const int* H, int nhid, const void* wout, const float* bout,
    const float* wbg, float* ey, int B, int S, int M, int Mpad, int N,
    int n_out, int act, int hidden_act, int is_bf16, int nsplit,
    hipStream_t stream);

// tree_kernels.hip
extern "C" int launch_fused_predict_trees(
    const uint8_t* masks, const int* vmap, const int64_t* dx, const int64_t* dbg,
    const uint8_t* child, const int* meta, const float* leaves,
    const int* grp_off, const int* grp_id, const int64_t* grp_mask,
    const float* base, const float* wbg, float* ey, float scale,
    int B, int S, int Mv, int N, int T, int G, int E, int L, int C,
    int max_internal, int n_out, int act, int leaf_mode, hipStream_t stream);

// tree_walk_kernels.hip
extern "C" int launch_fused_predict_trees_walk(
    const uint8_t* masks, const int* vmap, const float* x, const float* bg,
    const int* nodes, const int* roots, const float* leaves, const float* base,
    const float* wbg, float* ey, float scale,
    int B, int S, int Mv, int N, int D, int G, int T, int R, int L,
    int max_depth, int n_out, int act, int leaf_mode,
    const unsigned* cat_left, int C, hipStream_t stream);

// km_kernels.hip
extern "C" int launch_fused_predict_kernelmachine_pairs(
    const uint8_t* masks, const float* xp, const float* bgpn,
    const float* base, const float* alpha, const float* icpt,
    const float* prob_a, const float* prob_b, const float* wbg, float* ey,
    int B, int S, int M, int Mpad, int N, int Vpad, int n_classes,
    int n_pairs, int act, int kernel, float gamma, float coef0, int degree,
    hipStream_t stream);
extern "C" int launch_fused_predict_kernelmachine(
    const uint8_t* masks, const float* xp, const float* bgpn,
    const float* base, const float* alpha, const float* icpt,
    const float* wbg, float* ey, int B, int S, int M, int Mpad, int N,
    int Vpad, int n_out, int act, int kernel, float gamma, float coef0,
    int degree, hipStream_t stream);

namespace {

#define CHECK_DEV(t) TORCH_CHECK((t).is_cuda() && (t).is_contiguous(), #t " must be a contiguous device tensor")

hipStream_t current_stream() {
    return c10::hip::getCurrentHIPStream().stream();
}

void fill_random_masks(
    torch::Tensor masks, int64_t ne, int64_t n_random,
    torch::Tensor cdf, torch::Tensor sizes, int64_t num_paired, int64_t seed,
    torch::Tensor inst_ids) {
    CHECK_DEV(masks); CHECK_DEV(cdf); CHECK_DEV(sizes); CHECK_DEV(inst_ids);
    TORCH_CHECK(masks.dtype() == torch::kUInt8, "masks must be uint8");
    TORCH_CHECK(masks.dim() == 3, "masks must be (B,S,M)");
    TORCH_CHECK(inst_ids.dtype() == torch::kInt32, "inst_ids must be int32");
    int B = masks.size(0), S = masks.size(1), M = masks.size(2);
    TORCH_CHECK(inst_ids.size(0) == B, "inst_ids length");
    TORCH_CHECK(M <= 256, "fill_random_masks supports M <= 256");
    launch_fill_random_masks(
        masks.data_ptr<uint8_t>(), B, S, M, (int)ne, (int)n_random,
        cdf.data_ptr<float>(), sizes.data_ptr<int>(), (int)cdf.size(0),
        (int)num_paired, (uint32_t)seed, inst_ids.data_ptr<int32_t>(),
        current_stream());
}

void fused_predict_linear(
    torch::Tensor masks, torch::Tensor diff, torch::Tensor base,
    torch::Tensor wbg, torch::Tensor ey, int64_t act) {
    CHECK_DEV(masks); CHECK_DEV(diff); CHECK_DEV(base); CHECK_DEV(wbg); CHECK_DEV(ey);
    TORCH_CHECK(masks.dtype() == torch::kUInt8, "masks must be u8 (B,S,M)");
    int B = masks.size(0), S = masks.size(1), M = masks.size(2);
    int Mpad = diff.size(2), Npad = diff.size(3);
    int n_out = ey.size(2);                    // act 3 uses 1 diff image for 2 outputs
    int oimg = (act == 3) ? 1 : n_out;
    TORCH_CHECK(diff.size(1) == oimg, "diff image count vs act");
    TORCH_CHECK(M <= Mpad, "M vs Mpad");
    TORCH_CHECK(ey.size(0) == B && ey.size(1) == S, "ey shape");
    TORCH_CHECK(base.size(0) == oimg && base.size(1) == Npad, "base shape");
    TORCH_CHECK(wbg.size(0) == Npad, "wbg shape");
    int rc = launch_fused_predict_linear(
        masks.data_ptr<uint8_t>(), diff.data_ptr<float>(), base.data_ptr<float>(),
        wbg.data_ptr<float>(), ey.data_ptr<float>(), B, S, M, Mpad, Npad,
        n_out, (int)act, current_stream());
    TORCH_CHECK(rc == 0, "fused_predict_linear: unsupported shape (Mpad<=64, Npad%16==0, Npad<=128, n_out in {1,2,4})");
}

void fused_predict_linear_wide(
    torch::Tensor masks, torch::Tensor diff, torch::Tensor base,
    torch::Tensor wbg, torch::Tensor ey, int64_t act) {
    CHECK_DEV(masks); CHECK_DEV(diff); CHECK_DEV(base); CHECK_DEV(wbg); CHECK_DEV(ey);
    TORCH_CHECK(masks.dtype() == torch::kUInt8, "masks must be u8 (B,S,M)");
    TORCH_CHECK(diff.dtype() == torch::kFloat32 && base.dtype() == torch::kFloat32
                && wbg.dtype() == torch::kFloat32 && ey.dtype() == torch::kFloat32,
                "diff, base, wbg and ey must be float32");
    TORCH_CHECK(masks.dim() == 3 && diff.dim() == 4 && base.dim() == 2
                && wbg.dim() == 1 && ey.dim() == 3, "operand ranks");
    int B = masks.size(0), S = masks.size(1), M = masks.size(2);
    int noutp = diff.size(1), Mpad = diff.size(2), Npad = diff.size(3);
    int n_out = ey.size(2);                    // real classes; noutp images
    TORCH_CHECK(diff.size(0) == B, "diff batch");
    TORCH_CHECK(M <= Mpad, "M vs Mpad");
    TORCH_CHECK(ey.size(0) == B && ey.size(1) == S, "ey shape");
    TORCH_CHECK(base.size(0) == noutp && base.size(1) == Npad, "base shape");
    TORCH_CHECK(wbg.size(0) == Npad, "wbg shape");
    // the column-tile slices are staged with 16-byte loads
    TORCH_CHECK(reinterpret_cast<uintptr_t>(diff.data_ptr<float>()) % 16 == 0,
                "diff must be 16-byte aligned");
    int rc = launch_fused_predict_linear_wide(
        masks.data_ptr<uint8_t>(), diff.data_ptr<float>(), base.data_ptr<float>(),
        wbg.data_ptr<float>(), ey.data_ptr<float>(), B, S, M, Mpad, Npad,
        n_out, noutp, (int)act, current_stream());
    TORCH_CHECK(rc != -2, "fused_predict_linear_wide: the kernel launch was "
                "rejected by the runtime");
    TORCH_CHECK(rc == 0, "fused_predict_linear_wide: unsupported shape "
                "(act in {0,1,2}, 3<=n_out<=16 with ceil4(n_out) diff images, "
                "Mpad%4==0, Mpad<=64, Npad%16==0, Npad<=512)");
}

void synth_chunk(
    torch::Tensor masks, torch::Tensor x, torch::Tensor bg,
    torch::Tensor col_group, torch::Tensor out, int64_t b_lo, int64_t b_hi,
    int64_t s_lo, int64_t s_hi) {
    CHECK_DEV(masks); CHECK_DEV(x); CHECK_DEV(bg); CHECK_DEV(col_group); CHECK_DEV(out);
    int S = masks.size(1), M = masks.size(2);
    int N = bg.size(0), D = bg.size(1);
    TORCH_CHECK(out.size(0) == (b_hi - b_lo) * (s_hi - s_lo) * N && out.size(1) == D,
                "out shape");
    const bool bf16 = out.dtype() == torch::kBFloat16;
    TORCH_CHECK(bf16 || out.dtype() == torch::kFloat32,
                "out must be float32 or bfloat16");
    launch_synth_chunk(
        masks.data_ptr<uint8_t>(), x.data_ptr<float>(), bg.data_ptr<float>(),
        col_group.data_ptr<int>(),
        bf16 ? (void*)out.data_ptr<at::BFloat16>()
             : (void*)out.data_ptr<float>(),
        bf16 ? 1 : 0, S, M, N, D,
        (int)b_lo, (int)b_hi, (int)s_lo, (int)s_hi, current_stream());
}

void wls_solve(
    torch::Tensor masks, torch::Tensor kw, torch::Tensor ey_adj,
    torch::Tensor total, torch::Tensor phi,
    c10::optional<torch::Tensor> packed) {
    CHECK_DEV(masks); CHECK_DEV(kw); CHECK_DEV(ey_adj); CHECK_DEV(total); CHECK_DEV(phi);
    int B = masks.size(0), S = masks.size(1), M = masks.size(2);
    int n_out = ey_adj.size(2);
    TORCH_CHECK(phi.size(0) == B && phi.size(1) == M && phi.size(2) == n_out, "phi shape");
    const uint64_t* pk = nullptr;
    if (packed.has_value()) {
        CHECK_DEV(packed.value());
        TORCH_CHECK(packed->size(0) == B && packed->size(1) == S, "packed shape");
        pk = reinterpret_cast<const uint64_t*>(packed->data_ptr<int64_t>());
    }
    int rc = launch_wls_solve(
        masks.data_ptr<uint8_t>(), pk, kw.data_ptr<float>(), ey_adj.data_ptr<float>(),
        total.data_ptr<float>(), phi.data_ptr<float>(), B, S, M, n_out,
        current_stream());
    TORCH_CHECK(rc == 0, "wls_solve: unsupported shape (2<=M<=64, n_out<=8)");
}

void pack_masks(torch::Tensor masks, torch::Tensor packed) {
    CHECK_DEV(masks); CHECK_DEV(packed);
    TORCH_CHECK(masks.dtype() == torch::kUInt8, "masks must be u8");
    int B = masks.size(0), S = masks.size(1), M = masks.size(2);
    TORCH_CHECK(M <= 64, "pack_masks supports M <= 64");
    TORCH_CHECK(packed.size(0) == B && packed.size(1) == S, "packed shape");
    launch_pack_masks(
        masks.data_ptr<uint8_t>(),
        reinterpret_cast<uint64_t*>(packed.data_ptr<int64_t>()),
        B, S, M, current_stream());
}

#define CHECK_F32(t) TORCH_CHECK((t).dtype() == torch::kFloat32, #t " must be float32")
#define CHECK_I64(t) TORCH_CHECK((t).dtype() == torch::kInt64, #t " must be int64")

void fill_masks_packed(
    torch::Tensor packed, torch::Tensor enum_packed, int64_t n_random,
    torch::Tensor cdf, torch::Tensor sizes, int64_t num_paired, int64_t seed,
    torch::Tensor inst_ids, int64_t M) {
    CHECK_DEV(packed); CHECK_DEV(enum_packed); CHECK_DEV(cdf); CHECK_DEV(sizes);
    CHECK_DEV(inst_ids);
    CHECK_I64(packed); CHECK_I64(enum_packed); CHECK_F32(cdf);
    TORCH_CHECK(sizes.dtype() == torch::kInt32, "sizes must be int32");
    TORCH_CHECK(inst_ids.dtype() == torch::kInt32, "inst_ids must be int32");
    TORCH_CHECK(packed.dim() == 2 && enum_packed.dim() == 1,
                "packed must be (B,S), enum_packed (ne,)");
    int B = packed.size(0), S = packed.size(1), ne = enum_packed.size(0);
    TORCH_CHECK(inst_ids.dim() == 1 && inst_ids.size(0) == B, "inst_ids length");
    TORCH_CHECK(n_random >= 0 && ne + n_random == S, "ne + n_random must equal S");
    TORCH_CHECK(cdf.dim() == 1 && sizes.dim() == 1
                && cdf.size(0) == sizes.size(0), "cdf vs sizes");
    TORCH_CHECK(n_random == 0 || cdf.size(0) >= 1, "empty size table");
    int rc = launch_fill_masks_packed(
        reinterpret_cast<uint64_t*>(packed.data_ptr<int64_t>()),
        reinterpret_cast<const uint64_t*>(enum_packed.data_ptr<int64_t>()),
        B, S, (int)M, ne, (int)n_random, cdf.data_ptr<float>(),
        sizes.data_ptr<int>(), (int)cdf.size(0), (int)num_paired,
        (uint32_t)seed, inst_ids.data_ptr<int32_t>(), current_stream());
    TORCH_CHECK(rc == 0, "fill_masks_packed: unsupported shape (1<=M<=64)");
}

void linear_prepare(
    torch::Tensor X, torch::Tensor W, torch::Tensor bias,
    torch::Tensor col_group, torch::Tensor vidx, torch::Tensor bgp,
    torch::Tensor lfnull64, torch::Tensor diff, torch::Tensor total,
    int64_t act, int64_t link) {
    CHECK_DEV(X); CHECK_DEV(W); CHECK_DEV(bias); CHECK_DEV(col_group);
    CHECK_DEV(vidx); CHECK_DEV(bgp); CHECK_DEV(lfnull64); CHECK_DEV(diff);
    CHECK_DEV(total);
    CHECK_F32(X); CHECK_F32(W); CHECK_F32(bias); CHECK_F32(bgp); CHECK_F32(diff);
    CHECK_F32(total); CHECK_I64(col_group); CHECK_I64(vidx);
    TORCH_CHECK(lfnull64.dtype() == torch::kFloat64, "lfnull64 must be float64");
    TORCH_CHECK(X.dim() == 2 && W.dim() == 2 && bgp.dim() == 3 && diff.dim() == 4
                && total.dim() == 2 && vidx.dim() == 1, "operand ranks");
    int B = X.size(0), D = X.size(1), n_out = W.size(0);
    int N = bgp.size(0), G = bgp.size(1), OI = bgp.size(2), m = vidx.size(0);
    int Mpad = diff.size(2), Npad = diff.size(3);
    TORCH_CHECK(W.size(1) == D && bias.numel() == n_out
                && col_group.numel() == D && lfnull64.numel() == n_out,
                "W (n_out,D), b (n_out), col_group (D), lfnull64 (n_out)");
    TORCH_CHECK(OI == (act == 3 ? 1 : n_out), "background image count vs act");
    TORCH_CHECK(diff.size(0) == B && diff.size(1) == OI, "diff (B,OI,Mpad,Npad)");
    TORCH_CHECK(total.size(0) == B && total.size(1) == n_out, "total (B,n_out)");
    TORCH_CHECK(link == 0 || link == 1, "link must be 0 or 1");
    int rc = launch_linear_prepare(
        X.data_ptr<float>(), W.data_ptr<float>(), bias.data_ptr<float>(),
        col_group.data_ptr<int64_t>(), vidx.data_ptr<int64_t>(),
        bgp.data_ptr<float>(), lfnull64.data_ptr<double>(),
        diff.data_ptr<float>(), total.data_ptr<float>(), B, D, G, N, m, Mpad,
        Npad, n_out, (int)act, (int)link, current_stream());
    TORCH_CHECK(rc == 0, "linear_prepare: unsupported shape (m<=Mpad, m<=64, "
                         "N<=Npad, n_out<=8, act 3 needs n_out==2)");
}

void fused_predict_linear_packed(
    torch::Tensor packed, torch::Tensor diff, torch::Tensor base,
    torch::Tensor wbg, torch::Tensor ey, int64_t act, int64_t link,
    c10::optional<torch::Tensor> lfnull, int64_t mma) {
    CHECK_DEV(packed); CHECK_DEV(diff); CHECK_DEV(base); CHECK_DEV(wbg); CHECK_DEV(ey);
    CHECK_I64(packed); CHECK_F32(diff); CHECK_F32(base); CHECK_F32(wbg); CHECK_F32(ey);
    TORCH_CHECK(packed.dim() == 2 && diff.dim() == 4 && ey.dim() == 3
                && base.dim() == 2, "operand ranks");
    int B = packed.size(0), S = packed.size(1);
    int Mpad = diff.size(2), Npad = diff.size(3);
    int n_out = ey.size(2);
    int oimg = (act == 3) ? 1 : n_out;
    TORCH_CHECK(diff.size(0) == B && diff.size(1) == oimg, "diff (B,oimg,Mpad,Npad) vs act");
    TORCH_CHECK(ey.size(0) == B && ey.size(1) == S, "ey shape");
    TORCH_CHECK(base.size(0) == oimg && base.size(1) == Npad, "base shape");
    TORCH_CHECK(wbg.numel() == Npad, "wbg shape");
    const float* lf = nullptr;
    if (lfnull.has_value()) {
        CHECK_DEV(lfnull.value()); CHECK_F32(lfnull.value());
        TORCH_CHECK(lfnull->numel() == n_out, "lfnull must be (n_out,)");
        lf = lfnull->data_ptr<float>();
    }
    TORCH_CHECK(link == 0 || (link == 1 && lf != nullptr),
                "link must be 0, or 1 with lfnull given");
    TORCH_CHECK(mma >= -1 && mma <= 1,
                "mma must be -1 (auto), 0 (fp32 MFMA) or 1 (split bf16 MFMA)");
    int rc = launch_fused_predict_linear_packed(
        reinterpret_cast<const uint64_t*>(packed.data_ptr<int64_t>()),
        diff.data_ptr<float>(), base.data_ptr<float>(), wbg.data_ptr<float>(),
        lf, ey.data_ptr<float>(), B, S, Mpad, Npad, n_out, (int)act, (int)link,
        current_stream(), (int)mma);
    TORCH_CHECK(rc == 0, "fused_predict_linear_packed: unsupported shape "
                         "(Mpad%4==0, Mpad<=64, Npad%16==0, Npad<=128, n_out in "
                         "{1,2,4}, operand images within 64 KiB of LDS)");
}

void wls_solve_packed(
    torch::Tensor packed, torch::Tensor kw, torch::Tensor ey_adj,
    torch::Tensor total, torch::Tensor vidx, torch::Tensor phi_full) {
    CHECK_DEV(packed); CHECK_DEV(kw); CHECK_DEV(ey_adj); CHECK_DEV(total);
    CHECK_DEV(vidx); CHECK_DEV(phi_full);
    CHECK_I64(packed); CHECK_F32(kw); CHECK_F32(ey_adj); CHECK_F32(total);
    CHECK_I64(vidx); CHECK_F32(phi_full);
    TORCH_CHECK(packed.dim() == 2 && ey_adj.dim() == 3 && phi_full.dim() == 3
                && vidx.dim() == 1 && total.dim() == 2, "operand ranks");
    int B = packed.size(0), S = packed.size(1), M = vidx.size(0);
    int n_out = ey_adj.size(2), G = phi_full.size(1);
    TORCH_CHECK(kw.numel() == S, "kw must be (S,)");
    TORCH_CHECK(ey_adj.size(0) == B && ey_adj.size(1) == S, "ey_adj shape");
    TORCH_CHECK(total.size(0) == B && total.size(1) == n_out, "total shape");
    TORCH_CHECK(phi_full.size(0) == B && phi_full.size(2) == n_out, "phi_full shape");
    int rc = launch_wls_solve_packed(
        reinterpret_cast<const uint64_t*>(packed.data_ptr<int64_t>()),
        kw.data_ptr<float>(), ey_adj.data_ptr<float>(), total.data_ptr<float>(),
        vidx.data_ptr<int64_t>(), phi_full.data_ptr<float>(), B, S, M, n_out,
        G, current_stream());
    TORCH_CHECK(rc == 0, "wls_solve_packed: unsupported shape (2<=M<=G, "
                         "(M-1)+n_out<=16)");
}

void varying_probe(
    torch::Tensor X, torch::Tensor bg_min, torch::Tensor bg_max,
    torch::Tensor tol_min, torch::Tensor tol_max, torch::Tensor col_group,
    int64_t n_groups, torch::Tensor keys, torch::Tensor probe) {
    CHECK_DEV(X); CHECK_DEV(bg_min); CHECK_DEV(bg_max); CHECK_DEV(tol_min);
    CHECK_DEV(tol_max); CHECK_DEV(col_group); CHECK_DEV(keys); CHECK_DEV(probe);
    CHECK_F32(X); CHECK_F32(bg_min); CHECK_F32(bg_max); CHECK_F32(tol_min);
    CHECK_F32(tol_max); CHECK_I64(col_group); CHECK_I64(keys); CHECK_I64(probe);
    TORCH_CHECK(X.dim() == 2, "X must be (B,D)");
    const int64_t B = X.size(0), D = X.size(1);
    TORCH_CHECK(B >= 1 && D >= 1 && B <= 0x7fffffffLL && D <= 0x7fffffffLL,
                "X must be (B,D) with B, D >= 1");
    TORCH_CHECK(bg_min.numel() == D && bg_max.numel() == D
                && tol_min.numel() == D && tol_max.numel() == D
                && col_group.numel() == D,
                "bg_min, bg_max, tol_min, tol_max, col_group must be (D,)");
    TORCH_CHECK(keys.numel() == B, "keys must be (B,)");
    TORCH_CHECK(probe.numel() == 2, "probe must be (2,)");
    int rc = launch_varying_probe(
        X.data_ptr<float>(), bg_min.data_ptr<float>(), bg_max.data_ptr<float>(),
        tol_min.data_ptr<float>(), tol_max.data_ptr<float>(),
        col_group.data_ptr<int64_t>(), keys.data_ptr<int64_t>(),
        probe.data_ptr<int64_t>(), (int)B, (int)D, (int)n_groups,
        current_stream());
    TORCH_CHECK(rc == 0, "varying_probe: unsupported shape (1 <= n_groups <= 62)");
}

void fused_predict_bf16(
    torch::Tensor masks, torch::Tensor diffB, torch::Tensor base,
    torch::Tensor wbg, torch::Tensor ey, int64_t act) {
    CHECK_DEV(masks); CHECK_DEV(diffB); CHECK_DEV(base); CHECK_DEV(wbg); CHECK_DEV(ey);
    TORCH_CHECK(masks.dtype() == torch::kUInt8 && diffB.dtype() == torch::kBFloat16);
    int B = masks.size(0), S = masks.size(1), M = masks.size(2);
    int split = diffB.size(1), Npad = diffB.size(3);
    int n_out = ey.size(2);                    // act 3 uses 1 diff image for 2 outputs
    TORCH_CHECK(diffB.size(2) == ((act == 3) ? 1 : n_out), "diffB image count vs act");
    TORCH_CHECK(diffB.size(0) == B && diffB.size(4) == 40, "diffB (B,split,o,Npad,40)");
    TORCH_CHECK(ey.size(0) == B && ey.size(1) == S, "ey shape");
    int rc = launch_fused_predict_bf16(
        masks.data_ptr<uint8_t>(),
        reinterpret_cast<const uint16_t*>(diffB.data_ptr<at::BFloat16>()),
        base.data_ptr<float>(), wbg.data_ptr<float>(), ey.data_ptr<float>(),
        B, S, M, Npad, n_out, (int)act, split, current_stream());
    TORCH_CHECK(rc == 0, "fused_predict_bf16: unsupported shape (M<=32, Npad<=128, n_out in {1,2,4}, split in {1,2})");
}

void build_diff_f32(torch::Tensor xp, torch::Tensor bgp, torch::Tensor vidx,
                    torch::Tensor out) {
    CHECK_DEV(xp); CHECK_DEV(bgp); CHECK_DEV(vidx); CHECK_DEV(out);
    int B = xp.size(0), G = xp.size(1), O = xp.size(2);
    int N = bgp.size(0), m = vidx.size(0);
    int Mpad = out.size(2), Npad = out.size(3);
    TORCH_CHECK(out.size(0) == B && out.size(1) == O && m <= Mpad && N <= Npad);
    launch_build_diff_f32(
        xp.data_ptr<float>(), bgp.data_ptr<float>(), vidx.data_ptr<int64_t>(),
        out.data_ptr<float>(), B, G, O, N, m, Mpad, Npad, current_stream());
}

void build_diff_bf16(torch::Tensor xp, torch::Tensor bgp, torch::Tensor vidx,
                     torch::Tensor out) {
    CHECK_DEV(xp); CHECK_DEV(bgp); CHECK_DEV(vidx); CHECK_DEV(out);
    TORCH_CHECK(out.dtype() == torch::kBFloat16 && out.size(4) == 40);
    int B = xp.size(0), G = xp.size(1), O = xp.size(2);
    int N = bgp.size(0), m = vidx.size(0);
    int split = out.size(1), Npad = out.size(3);
    TORCH_CHECK(out.size(0) == B && out.size(2) == O && N <= Npad && m <= 32);
    launch_build_diff_bf16(
        xp.data_ptr<float>(), bgp.data_ptr<float>(), vidx.data_ptr<int64_t>(),
        reinterpret_cast<uint16_t*>(out.data_ptr<at::BFloat16>()), B, G, O, N,
        m, Npad, split, current_stream());
}

void pack_masks_words(torch::Tensor masks, torch::Tensor packed) {
    CHECK_DEV(masks); CHECK_DEV(packed);
    TORCH_CHECK(masks.dtype() == torch::kUInt8, "masks must be u8");
    TORCH_CHECK(packed.dim() == 3, "packed must be (B,S,W)");
    int B = masks.size(0), S = masks.size(1), M = masks.size(2);
    int W = packed.size(2);
    TORCH_CHECK(packed.size(0) == B && packed.size(1) == S, "packed shape");
    TORCH_CHECK(W * 64 >= M, "packed word count vs M");
    launch_pack_masks_words(
        masks.data_ptr<uint8_t>(),
        reinterpret_cast<uint64_t*>(packed.data_ptr<int64_t>()),
        B, S, M, W, current_stream());
}

void wls_gram(
    torch::Tensor packed, torch::Tensor kw, torch::Tensor ey_adj,
    torch::Tensor total, torch::Tensor A64, torch::Tensor rhs64) {
    CHECK_DEV(packed); CHECK_DEV(kw); CHECK_DEV(ey_adj); CHECK_DEV(total);
    CHECK_DEV(A64); CHECK_DEV(rhs64);
    TORCH_CHECK(packed.dim() == 3, "packed must be (B,S,W)");
    TORCH_CHECK(A64.dtype() == torch::kFloat64 && rhs64.dtype() == torch::kFloat64);
    int B = packed.size(0), S = packed.size(1), W = packed.size(2);
    int mm = A64.size(1), n_out = ey_adj.size(2);
    TORCH_CHECK(A64.size(0) == B && A64.size(2) == mm, "A64 shape");
    TORCH_CHECK(rhs64.size(0) == B && rhs64.size(1) == mm
                && rhs64.size(2) == n_out, "rhs64 shape");
    TORCH_CHECK(W * 64 >= mm + 1, "packed word count vs M");
    int rc = launch_wls_gram(
        reinterpret_cast<const uint64_t*>(packed.data_ptr<int64_t>()),
        kw.data_ptr<float>(), ey_adj.data_ptr<float>(),
        total.data_ptr<float>(), A64.data_ptr<double>(),
        rhs64.data_ptr<double>(), B, S, mm + 1, W, n_out, current_stream());
    TORCH_CHECK(rc == 0, "wls_gram: unsupported shape (M<=513, n_out<=8)");
}

void fused_predict_tiled(
    torch::Tensor masks, torch::Tensor diff, torch::Tensor base,
    torch::Tensor wbg, torch::Tensor partial, torch::Tensor ey, int64_t act) {
    CHECK_DEV(masks); CHECK_DEV(diff); CHECK_DEV(base); CHECK_DEV(wbg);
    CHECK_DEV(partial); CHECK_DEV(ey);
    TORCH_CHECK(masks.dtype() == torch::kUInt8, "masks must be u8 (B,S,M)");
    int B = masks.size(0), S = masks.size(1), M = masks.size(2);
    int Mpad = diff.size(2), Npad = diff.size(3);
    int n_out = ey.size(2);
    int oimg = (act == 3) ? 1 : n_out;
    int nacc = n_out;   // act 3 dual-accumulates p0 and p1
    int n_ntiles = (Npad + 127) / 128;
    TORCH_CHECK(diff.size(1) == oimg, "diff image count vs act");
    TORCH_CHECK(M <= Mpad, "M vs Mpad");
    TORCH_CHECK(ey.size(0) == B && ey.size(1) == S, "ey shape");
    TORCH_CHECK(base.size(0) == oimg && base.size(1) == Npad, "base shape");
    TORCH_CHECK(wbg.size(0) == Npad, "wbg shape");
    TORCH_CHECK(partial.size(0) == B && partial.size(1) == n_ntiles
                && partial.size(2) == S && partial.size(3) == nacc,
                "partial shape (B, n_ntiles, S, nacc)");
    int rc = launch_fused_predict_tiled(
        masks.data_ptr<uint8_t>(), diff.data_ptr<float>(),
        base.data_ptr<float>(), wbg.data_ptr<float>(),
        partial.data_ptr<float>(), ey.data_ptr<float>(), B, S, M, Mpad,
        Npad, n_out, (int)act, current_stream());
    TORCH_CHECK(rc == 0, "fused_predict_tiled: unsupported shape "
                         "(Mpad%16==0, Npad%16==0, n_out in {1,2,4})");
}

void build_diff_bf16_tiled(torch::Tensor xp, torch::Tensor bgp,
                           torch::Tensor vidx, torch::Tensor out) {
    CHECK_DEV(xp); CHECK_DEV(bgp); CHECK_DEV(vidx); CHECK_DEV(out);
    TORCH_CHECK(out.dtype() == torch::kBFloat16 && out.dim() == 5,
                "out must be bf16 (B,split,O,Npad,Mpad)");
    int B = xp.size(0), G = xp.size(1), O = xp.size(2);
    int N = bgp.size(0), mcount = vidx.size(0);
    int split = out.size(1), Npad = out.size(3), Mpad = out.size(4);
    TORCH_CHECK(out.size(0) == B && out.size(2) == O && N <= Npad
                && mcount <= Mpad);
    launch_build_diff_bf16_tiled(
        xp.data_ptr<float>(), bgp.data_ptr<float>(), vidx.data_ptr<int64_t>(),
        reinterpret_cast<uint16_t*>(out.data_ptr<at::BFloat16>()), B, G, O, N,
        mcount, Mpad, Npad, split, current_stream());
}

void fused_predict_tiled_bf16(
    torch::Tensor masks, torch::Tensor diffB, torch::Tensor base,
    torch::Tensor wbg, torch::Tensor partial, torch::Tensor ey, int64_t act) {
    CHECK_DEV(masks); CHECK_DEV(diffB); CHECK_DEV(base); CHECK_DEV(wbg);
    CHECK_DEV(partial); CHECK_DEV(ey);
    TORCH_CHECK(masks.dtype() == torch::kUInt8
                && diffB.dtype() == torch::kBFloat16);
    int B = masks.size(0), S = masks.size(1), M = masks.size(2);
    int split = diffB.size(1), Npad = diffB.size(3), Mpad = diffB.size(4);
    int n_out = ey.size(2);
    int oimg = (act == 3) ? 1 : n_out;
    int n_ntiles = (Npad + 127) / 128;
    TORCH_CHECK(diffB.size(2) == oimg, "diffB image count vs act");
    TORCH_CHECK(ey.size(0) == B && ey.size(1) == S, "ey shape");
    TORCH_CHECK(base.size(0) == oimg && base.size(1) == Npad, "base shape");
    TORCH_CHECK(wbg.size(0) == Npad, "wbg shape");
    TORCH_CHECK(partial.size(0) == B && partial.size(1) == n_ntiles
                && partial.size(2) == S && partial.size(3) == n_out,
                "partial shape");
    TORCH_CHECK((size_t)split * oimg * 128 * 40 * 2 <= 64 * 1024,
                "bf16 tiled LDS footprint (split*oimg too large)");
    int rc = launch_fused_predict_tiled_bf16(
        masks.data_ptr<uint8_t>(),
        reinterpret_cast<const uint16_t*>(diffB.data_ptr<at::BFloat16>()),
        base.data_ptr<float>(), wbg.data_ptr<float>(),
        partial.data_ptr<float>(), ey.data_ptr<float>(), B, S, M, Mpad, Npad,
        n_out, (int)act, split, current_stream());
    TORCH_CHECK(rc == 0, "fused_predict_tiled_bf16: unsupported shape "
                         "(Mpad%32==0, Npad%16==0, n_out in {1,2,4})");
}

void fused_predict_mlp(
    torch::Tensor masks, torch::Tensor xp1, torch::Tensor bgp1n,
    torch::Tensor base1, std::vector<torch::Tensor> hidden_w,
    std::vector<torch::Tensor> hidden_b, torch::Tensor wout,
    torch::Tensor bout, torch::Tensor wbg, torch::Tensor ey, int64_t act,
    int64_t hidden_act) {
    static const char* envelope =
        "fused_predict_mlp: outside the supported envelope (1-3 relu hidden "
        "layers of padded width <= 256, n_out <= 8, M <= Mpad <= 64, widths "
        "padded to 16 (fp32) / 32 (bf16))";
    CHECK_DEV(masks); CHECK_DEV(xp1); CHECK_DEV(bgp1n); CHECK_DEV(base1);
    CHECK_DEV(wout); CHECK_DEV(bout); CHECK_DEV(wbg); CHECK_DEV(ey);
    TORCH_CHECK(masks.dtype() == torch::kUInt8 && masks.dim() == 3,
                "masks must be u8 (B,S,M)");
    const bool bf16 = xp1.dtype() == torch::kBFloat16;
    TORCH_CHECK(bf16 || xp1.dtype() == torch::kFloat32,
                "operand images must be float32 or bfloat16");
    const auto wdt = xp1.dtype();
    TORCH_CHECK(hidden_w.size() == hidden_b.size(), "hidden_w vs hidden_b");
    TORCH_CHECK(hidden_w.size() + 1 <= 3, envelope);
    const int nhid = (int)hidden_w.size() + 1;
    TORCH_CHECK(xp1.dim() == 3 && bgp1n.dim() == 3 && base1.dim() == 2
                && wout.dim() == 3 && ey.dim() == 3, "operand ranks");
    int B = masks.size(0), S = masks.size(1), M = masks.size(2);
    int H[3] = {(int)xp1.size(1), 0, 0};
    int Mpad = xp1.size(2), N = bgp1n.size(0), n_out = ey.size(2);
    TORCH_CHECK(xp1.size(0) == B, "xp1 must be (B,H1,Mpad)");
    TORCH_CHECK(bgp1n.dtype() == wdt && bgp1n.size(1) == H[0]
                && bgp1n.size(2) == Mpad, "bgp1n must be (N,H1,Mpad)");
    TORCH_CHECK(base1.dtype() == torch::kFloat32 && base1.size(0) == N
                && base1.size(1) == H[0], "base1 must be f32 (N,H1)");
    const void* hw[2] = {nullptr, nullptr};
    const float* hb[2] = {nullptr, nullptr};
    for (int l = 1; l < nhid; ++l) {
        const torch::Tensor& w = hidden_w[l - 1];
        const torch::Tensor& bb = hidden_b[l - 1];
        CHECK_DEV(w); CHECK_DEV(bb);
        TORCH_CHECK(w.dtype() == wdt && w.dim() == 2 && w.size(1) == H[l - 1],
                    "hidden weight must be (H_out, H_in) in the operand dtype");
        H[l] = w.size(0);
        TORCH_CHECK(bb.dtype() == torch::kFloat32 && bb.dim() == 1
                    && bb.size(0) == H[l], "hidden bias must be f32 (H_out)");
        hw[l - 1] = w.data_ptr();
        hb[l - 1] = bb.data_ptr<float>();
    }
    const int nsplit = wout.size(0);
    TORCH_CHECK(wout.dtype() == wdt && wout.size(1) == 16
                && wout.size(2) == H[nhid - 1], "wout must be (nsplit,16,H_last)");
    TORCH_CHECK(bout.dtype() == torch::kFloat32 && bout.numel() == 16,
                "bout must be f32 (16)");
    TORCH_CHECK(wbg.dtype() == torch::kFloat32 && wbg.numel() == N, "wbg must be f32 (N)");
    TORCH_CHECK(ey.dtype() == torch::kFloat32 && ey.size(0) == B
                && ey.size(1) == S, "ey must be f32 (B,S,n_out)");
    int rc = launch_fused_predict_mlp(
        masks.data_ptr<uint8_t>(), xp1.data_ptr(), bgp1n.data_ptr(),
        base1.data_ptr<float>(), hw, hb, H, nhid, wout.data_ptr(),
        bout.data_ptr<float>(), wbg.data_ptr<float>(), ey.data_ptr<float>(),
        B, S, M, Mpad, N, n_out, (int)act, (int)hidden_act, bf16 ? 1 : 0,
        nsplit, current_stream());
    TORCH_CHECK(rc != -2, "fused_predict_mlp: LDS size attribute rejected");
    TORCH_CHECK(rc == 0, envelope);
}

void fused_predict_trees(
    torch::Tensor masks, torch::Tensor vmap, torch::Tensor dx,
    torch::Tensor dbg, torch::Tensor child, torch::Tensor meta,
    torch::Tensor leaves, torch::Tensor grp_off, torch::Tensor grp_id,
    torch::Tensor grp_mask, torch::Tensor base, double scale,
    torch::Tensor wbg, torch::Tensor ey, int64_t act, int64_t leaf_mode,
    int64_t max_internal) {
    static const char* envelope =
        "fused_predict_trees: outside the supported envelope (1-1024 trees of "
        "at most 64 internal nodes each, n_out <= 8, 128 B per tree plus 2 B "
        "per internal node within 160 KiB of LDS)";
    CHECK_DEV(masks); CHECK_DEV(vmap); CHECK_DEV(dx); CHECK_DEV(dbg);
    CHECK_DEV(child); CHECK_DEV(meta); CHECK_DEV(leaves); CHECK_DEV(grp_off);
    CHECK_DEV(grp_id); CHECK_DEV(grp_mask); CHECK_DEV(base); CHECK_DEV(wbg);
    CHECK_DEV(ey);
    TORCH_CHECK(masks.dtype() == torch::kUInt8 && masks.dim() == 3,
                "masks must be u8 (B,S,Mv)");
    TORCH_CHECK(ey.dtype() == torch::kFloat32 && ey.dim() == 3,
                "ey must be f32 (B,S,n_out)");
    const int B = masks.size(0), S = masks.size(1), Mv = masks.size(2);
    const int n_out = ey.size(2);
    TORCH_CHECK(ey.size(0) == B && ey.size(1) == S, "ey must be f32 (B,S,n_out)");
    TORCH_CHECK(vmap.dtype() == torch::kInt32 && vmap.dim() == 1,
                "the group table must be int32 (G)");
    TORCH_CHECK(dx.dtype() == torch::kInt64 && dx.dim() == 2 && dx.size(0) == B,
                "dx must be int64 (B,T)");
    const int T = dx.size(1);
    TORCH_CHECK(dbg.dtype() == torch::kInt64 && dbg.dim() == 2
                && dbg.size(1) == T, "dbg must be int64 (N,T)");
    const int N = dbg.size(0);
    TORCH_CHECK(child.dtype() == torch::kUInt8 && child.dim() == 2
                && child.size(1) == 2, "child must be u8 (C,2)");
    TORCH_CHECK(meta.dtype() == torch::kInt32 && meta.dim() == 2
                && meta.size(0) == T && meta.size(1) == 4,
                "meta must be int32 (T,4)");
    TORCH_CHECK(leaf_mode == 0 || leaf_mode == 1, "leaf_mode must be 0 or 1");
    TORCH_CHECK(leaves.dtype() == torch::kFloat32
                && (leaf_mode == 0 ? leaves.dim() == 1
                                   : (leaves.dim() == 2 && leaves.size(1) == n_out)),
                "leaves must be f32 (L) for scalar or (L,n_out) for vector leaves");
    TORCH_CHECK(grp_off.dtype() == torch::kInt32 && grp_off.dim() == 1
                && grp_off.size(0) == T + 1, "grp_off must be int32 (T+1)");
    TORCH_CHECK(grp_id.dtype() == torch::kInt32 && grp_id.dim() == 1,
                "grp_id must be int32 (E)");
    TORCH_CHECK(grp_mask.dtype() == torch::kInt64 && grp_mask.dim() == 1
                && grp_mask.size(0) == grp_id.size(0), "grp_mask must be int64 (E)");
    TORCH_CHECK(base.dtype() == torch::kFloat32 && base.numel() == n_out,
                "base must be f32 (n_out)");
    TORCH_CHECK(wbg.dtype() == torch::kFloat32 && wbg.numel() == N,
                "wbg must be f32 (N)");
    TORCH_CHECK(max_internal <= 64 && max_internal >= 1, envelope);
    int rc = launch_fused_predict_trees(
        masks.data_ptr<uint8_t>(), vmap.data_ptr<int>(), dx.data_ptr<int64_t>(),
        dbg.data_ptr<int64_t>(), child.data_ptr<uint8_t>(), meta.data_ptr<int>(),
        leaves.data_ptr<float>(), grp_off.data_ptr<int>(), grp_id.data_ptr<int>(),
        grp_mask.data_ptr<int64_t>(), base.data_ptr<float>(),
        wbg.data_ptr<float>(), ey.data_ptr<float>(), (float)scale, B, S, Mv, N,
        T, (int)vmap.size(0), (int)grp_id.size(0), (int)leaves.size(0),
        (int)child.size(0), (int)max_internal, n_out, (int)act, (int)leaf_mode,
        current_stream());
    TORCH_CHECK(rc != -2, "fused_predict_trees: LDS size attribute rejected");
    TORCH_CHECK(rc == 0, envelope);
}

void fused_predict_trees_walk(
    torch::Tensor masks, torch::Tensor vmap, torch::Tensor x, torch::Tensor bg,
    torch::Tensor nodes, torch::Tensor roots, torch::Tensor leaves,
    torch::Tensor base, double scale, torch::Tensor wbg, torch::Tensor ey,
    int64_t act, int64_t leaf_mode, int64_t max_depth,
    c10::optional<torch::Tensor> cat_left) {
    static const char* envelope =
        "fused_predict_trees_walk: outside the supported envelope (depth <= "
        "64, n_out <= 8, at most 1024 groups and 4096 features, node records "
        "indexed by int32)";
    CHECK_DEV(masks); CHECK_DEV(vmap); CHECK_DEV(x); CHECK_DEV(bg);
    CHECK_DEV(nodes); CHECK_DEV(roots); CHECK_DEV(leaves); CHECK_DEV(base);
    CHECK_DEV(wbg); CHECK_DEV(ey);
    TORCH_CHECK(masks.dtype() == torch::kUInt8 && masks.dim() == 3,
                "masks must be u8 (B,S,Mv)");
    TORCH_CHECK(ey.dtype() == torch::kFloat32 && ey.dim() == 3,
                "ey must be f32 (B,S,n_out)");
    const int B = masks.size(0), S = masks.size(1), Mv = masks.size(2);
    const int n_out = ey.size(2);
    TORCH_CHECK(ey.size(0) == B && ey.size(1) == S, "ey must be f32 (B,S,n_out)");
    TORCH_CHECK(vmap.dtype() == torch::kInt32 && vmap.dim() == 1,
                "the group table must be int32 (G)");
    TORCH_CHECK(x.dtype() == torch::kFloat32 && x.dim() == 2 && x.size(0) == B,
                "x must be f32 (B,D)");
    const int64_t D = x.size(1);
    TORCH_CHECK(bg.dtype() == torch::kFloat32 && bg.dim() == 2
                && bg.size(1) == D, "bg must be f32 (N,D)");
    const int N = bg.size(0);
    TORCH_CHECK(nodes.dtype() == torch::kInt32 && nodes.dim() == 2
                && nodes.size(1) == 4, "nodes must be int32 (R,4)");
    TORCH_CHECK(roots.dtype() == torch::kInt32 && roots.dim() == 1,
                "roots must be int32 (T)");
    TORCH_CHECK(leaf_mode == 0 || leaf_mode == 1, "leaf_mode must be 0 or 1");
    TORCH_CHECK(leaves.dtype() == torch::kFloat32
                && (leaf_mode == 0 ? leaves.dim() == 1
                                   : (leaves.dim() == 2 && leaves.size(1) == n_out)),
                "leaves must be f32 (L) for scalar or (L,n_out) for vector leaves");
    TORCH_CHECK(base.dtype() == torch::kFloat32 && base.numel() == n_out,
                "base must be f32 (n_out)");
    TORCH_CHECK(wbg.dtype() == torch::kFloat32 && wbg.numel() == N,
                "wbg must be f32 (N)");
    TORCH_CHECK(max_depth >= 0 && max_depth <= 64, envelope);
    // routed tables: x and bg are encoded rows, cat_left the bitset rows
    const unsigned* cat_ptr = nullptr;
    int64_t C = 0;
    if (cat_left.has_value()) {
        const torch::Tensor& cl = *cat_left;
        CHECK_DEV(cl);
        TORCH_CHECK(cl.dtype() == torch::kInt32 && cl.dim() == 2
                    && cl.size(1) == 8 && cl.size(0) >= 1,
                    "cat_left must be int32 (C,8) with C >= 1");
        TORCH_CHECK(cl.size(0) <= 0x7fffffffLL / 8, envelope);
        cat_ptr = reinterpret_cast<const unsigned*>(cl.data_ptr<int>());
        C = cl.size(0);
    }
    TORCH_CHECK(nodes.size(0) <= 0x7fffffffLL && leaves.size(0) <= 0x7fffffffLL
                && roots.size(0) <= 0x7fffffffLL && D <= 0x7fffffffLL
                && vmap.size(0) <= 0x7fffffffLL, envelope);
    int rc = launch_fused_predict_trees_walk(
        masks.data_ptr<uint8_t>(), vmap.data_ptr<int>(), x.data_ptr<float>(),
        bg.data_ptr<float>(), nodes.data_ptr<int>(), roots.data_ptr<int>(),
        leaves.data_ptr<float>(), base.data_ptr<float>(), wbg.data_ptr<float>(),
        ey.data_ptr<float>(), (float)scale, B, S, Mv, N, (int)D,
        (int)vmap.size(0), (int)roots.size(0), (int)nodes.size(0),
        (int)leaves.size(0), (int)max_depth, n_out, (int)act, (int)leaf_mode,
        cat_ptr, (int)C, current_stream());
    TORCH_CHECK(rc != -2, "fused_predict_trees_walk: LDS size attribute rejected");
    TORCH_CHECK(rc == 0, envelope);
}

void fused_predict_kernelmachine(
    torch::Tensor masks, torch::Tensor xp, torch::Tensor bgpn,
    torch::Tensor base, torch::Tensor alpha, torch::Tensor intercept,
    torch::Tensor wbg, torch::Tensor ey, int64_t kernel, double gamma,
    double coef0, int64_t degree, int64_t act) {
    static const char* envelope =
        "fused_predict_kernelmachine: outside the supported envelope (rbf or "
        "poly of degree 1-8, at most 2048 support vectors after padding to "
        "16, n_out <= 8, M <= Mpad <= 64 with Mpad a multiple of 16)";
    CHECK_DEV(masks); CHECK_DEV(xp); CHECK_DEV(bgpn); CHECK_DEV(base);
    CHECK_DEV(alpha); CHECK_DEV(intercept); CHECK_DEV(wbg); CHECK_DEV(ey);
    TORCH_CHECK(masks.dtype() == torch::kUInt8 && masks.dim() == 3,
                "masks must be u8 (B,S,M)");
    TORCH_CHECK(xp.dtype() == torch::kFloat32 && xp.dim() == 3,
                "xp must be f32 (B,Vpad,Mpad)");
    const int B = masks.size(0), S = masks.size(1), M = masks.size(2);
    const int Vpad = xp.size(1), Mpad = xp.size(2);
    TORCH_CHECK(xp.size(0) == B, "xp must be f32 (B,Vpad,Mpad)");
    TORCH_CHECK(bgpn.dtype() == torch::kFloat32 && bgpn.dim() == 3
                && bgpn.size(1) == Vpad && bgpn.size(2) == Mpad,
                "bgpn must be f32 (N,Vpad,Mpad)");
    const int N = bgpn.size(0);
    TORCH_CHECK(base.dtype() == torch::kFloat32 && base.dim() == 2
                && base.size(0) == N && base.size(1) == Vpad,
                "base must be f32 (N,Vpad)");
    TORCH_CHECK(alpha.dtype() == torch::kFloat32 && alpha.dim() == 2
                && alpha.size(0) == 16 && alpha.size(1) == Vpad,
                "alpha must be f32 (16,Vpad)");
    TORCH_CHECK(intercept.dtype() == torch::kFloat32 && intercept.numel() == 16,
                "intercept must be f32 (16)");
    TORCH_CHECK(wbg.dtype() == torch::kFloat32 && wbg.numel() == N,
                "wbg must be f32 (N)");
    TORCH_CHECK(ey.dtype() == torch::kFloat32 && ey.dim() == 3
                && ey.size(0) == B && ey.size(1) == S,
                "ey must be f32 (B,S,n_out)");
    const int n_out = ey.size(2);
    int rc = launch_fused_predict_kernelmachine(
        masks.data_ptr<uint8_t>(), xp.data_ptr<float>(), bgpn.data_ptr<float>(),
        base.data_ptr<float>(), alpha.data_ptr<float>(),
        intercept.data_ptr<float>(), wbg.data_ptr<float>(),
        ey.data_ptr<float>(), B, S, M, Mpad, N, Vpad, n_out, (int)act,
        (int)kernel, (float)gamma, (float)coef0, (int)degree, current_stream());
    TORCH_CHECK(rc == 0, envelope);
}

void fused_predict_kernelmachine_pairs(
    torch::Tensor masks, torch::Tensor xp, torch::Tensor bgpn,
    torch::Tensor base, torch::Tensor alpha, torch::Tensor intercept,
    torch::Tensor prob_a, torch::Tensor prob_b, torch::Tensor wbg,
    torch::Tensor ey, int64_t kernel, double gamma, double coef0,
    int64_t degree, int64_t act, int64_t n_classes, int64_t n_pairs) {
    static const char* envelope =
        "fused_predict_kernelmachine_pairs: outside the supported envelope "
        "(rbf or poly of degree 1-8, at most 2048 support vectors after "
        "padding to 16, 3 to 6 classes with K(K-1)/2 pair rows, act 3 (ovr) "
        "or 4 (coupling), M <= Mpad <= 64 with Mpad a multiple of 16)";
    CHECK_DEV(masks); CHECK_DEV(xp); CHECK_DEV(bgpn); CHECK_DEV(base);
    CHECK_DEV(alpha); CHECK_DEV(intercept); CHECK_DEV(prob_a);
    CHECK_DEV(prob_b); CHECK_DEV(wbg); CHECK_DEV(ey);
    TORCH_CHECK(masks.dtype() == torch::kUInt8 && masks.dim() == 3,
                "masks must be u8 (B,S,M)");
    TORCH_CHECK(xp.dtype() == torch::kFloat32 && xp.dim() == 3,
                "xp must be f32 (B,Vpad,Mpad)");
    const int B = masks.size(0), S = masks.size(1), M = masks.size(2);
    const int Vpad = xp.size(1), Mpad = xp.size(2);
    TORCH_CHECK(xp.size(0) == B, "xp must be f32 (B,Vpad,Mpad)");
    TORCH_CHECK(bgpn.dtype() == torch::kFloat32 && bgpn.dim() == 3
                && bgpn.size(1) == Vpad && bgpn.size(2) == Mpad,
                "bgpn must be f32 (N,Vpad,Mpad)");
    const int N = bgpn.size(0);
    TORCH_CHECK(base.dtype() == torch::kFloat32 && base.dim() == 2
                && base.size(0) == N && base.size(1) == Vpad,
                "base must be f32 (N,Vpad)");
    TORCH_CHECK(alpha.dtype() == torch::kFloat32 && alpha.dim() == 2
                && alpha.size(0) == 16 && alpha.size(1) == Vpad,
                "alpha must be f32 (16,Vpad)");
    TORCH_CHECK(intercept.dtype() == torch::kFloat32 && intercept.numel() == 16,
                "intercept must be f32 (16)");
    TORCH_CHECK(prob_a.dtype() == torch::kFloat32 && prob_a.numel() == 16
                && prob_b.dtype() == torch::kFloat32 && prob_b.numel() == 16,
                "prob_a and prob_b must be f32 (16)");
    TORCH_CHECK(wbg.dtype() == torch::kFloat32 && wbg.numel() == N,
                "wbg must be f32 (N)");
    TORCH_CHECK(ey.dtype() == torch::kFloat32 && ey.dim() == 3
                && ey.size(0) == B && ey.size(1) == S
                && ey.size(2) == n_classes,
                "ey must be f32 (B,S,n_classes)");
    TORCH_CHECK(n_classes >= 0 && n_classes < (1 << 16) && n_pairs >= 0
                && n_pairs < (1 << 30), envelope);
    int rc = launch_fused_predict_kernelmachine_pairs(
        masks.data_ptr<uint8_t>(), xp.data_ptr<float>(), bgpn.data_ptr<float>(),
        base.data_ptr<float>(), alpha.data_ptr<float>(),
        intercept.data_ptr<float>(), prob_a.data_ptr<float>(),
        prob_b.data_ptr<float>(), wbg.data_ptr<float>(), ey.data_ptr<float>(),
        B, S, M, Mpad, N, Vpad, (int)n_classes, (int)n_pairs, (int)act,
        (int)kernel, (float)gamma, (float)coef0, (int)degree, current_stream());
    TORCH_CHECK(rc == 0, envelope);
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    m.def("fused_predict_kernelmachine_pairs", &fused_predict_kernelmachine_pairs,
          "fused one-vs-one kernel-machine predict (K4kp): the K4k main loop "
          "over K(K-1)/2 pair rows with a per-row epilogue (ovr votes or "
          "pairwise coupling) into K class scores",
          pybind11::arg("masks"), pybind11::arg("xp"), pybind11::arg("bgpn"),
          pybind11::arg("base"), pybind11::arg("alpha"),
          pybind11::arg("intercept"), pybind11::arg("prob_a"),
          pybind11::arg("prob_b"), pybind11::arg("wbg"), pybind11::arg("ey"),
          pybind11::arg("kernel"), pybind11::arg("gamma"),
          pybind11::arg("coef0"), pybind11::arg("degree"), pybind11::arg("act"),
          pybind11::arg("n_classes"), pybind11::arg("n_pairs"));
    m.def("fused_predict_kernelmachine", &fused_predict_kernelmachine,
          "fused kernel-machine predict (K4k): distance / dot product folded "
          "over varying groups, support vectors streamed in tiles of 16, "
          "kernel evaluation and the contraction with alpha on chip",
          pybind11::arg("masks"), pybind11::arg("xp"), pybind11::arg("bgpn"),
          pybind11::arg("base"), pybind11::arg("alpha"),
          pybind11::arg("intercept"), pybind11::arg("wbg"), pybind11::arg("ey"),
          pybind11::arg("kernel"), pybind11::arg("gamma"),
          pybind11::arg("coef0"), pybind11::arg("degree"), pybind11::arg("act"));
    m.def("fused_predict_trees", &fused_predict_trees,
          "fused tree-ensemble predict (K4t): per-tree node masks in LDS, "
          "bitwise select of packed x / background decisions, bit-register walk",
          pybind11::arg("masks"), pybind11::arg("vmap"), pybind11::arg("dx"),
          pybind11::arg("dbg"), pybind11::arg("child"), pybind11::arg("meta"),
          pybind11::arg("leaves"), pybind11::arg("grp_off"),
          pybind11::arg("grp_id"), pybind11::arg("grp_mask"),
          pybind11::arg("base"), pybind11::arg("scale"), pybind11::arg("wbg"),
          pybind11::arg("ey"), pybind11::arg("act"), pybind11::arg("leaf_mode"),
          pybind11::arg("max_internal"));
    m.def("fused_predict_trees_walk", &fused_predict_trees_walk,
          "fused deep-tree predict (K4w): 16-byte node records walked on the "
          "blended row, group bitset per sample, x row and background in LDS",
          pybind11::arg("masks"), pybind11::arg("vmap"), pybind11::arg("x"),
          pybind11::arg("bg"), pybind11::arg("nodes"), pybind11::arg("roots"),
          pybind11::arg("leaves"), pybind11::arg("base"),
          pybind11::arg("scale"), pybind11::arg("wbg"), pybind11::arg("ey"),
          pybind11::arg("act"), pybind11::arg("leaf_mode"),
          pybind11::arg("max_depth"),
          pybind11::arg("cat_left") = pybind11::none());
    m.def("fused_predict_mlp", &fused_predict_mlp,
          "fused MLP predict (K4m): first layer folded over varying groups, "
          "hidden activations in LDS, f32 or bf16 MFMA by operand dtype",
          pybind11::arg("masks"), pybind11::arg("xp1"), pybind11::arg("bgp1n"),
          pybind11::arg("base1"), pybind11::arg("hidden_w"),
          pybind11::arg("hidden_b"), pybind11::arg("wout"),
          pybind11::arg("bout"), pybind11::arg("wbg"), pybind11::arg("ey"),
          pybind11::arg("act"), pybind11::arg("hidden_act") = 0);
    m.def("fill_masks_packed", &fill_masks_packed,
          "Philox coalition sampling straight into packed u64 words (K2p): "
          "bit-identical to the enumerated-row copy, fill_random_masks and "
          "pack_masks in sequence, M <= 64",
          pybind11::arg("packed"), pybind11::arg("enum_packed"),
          pybind11::arg("n_random"), pybind11::arg("cdf"),
          pybind11::arg("sizes"), pybind11::arg("num_paired"),
          pybind11::arg("seed"), pybind11::arg("inst_ids"), pybind11::arg("M"));
    m.def("linear_prepare", &linear_prepare,
          "per-call operand prep for the packed linear pipeline (K0p): diff "
          "image in the build_diff_f32 layout plus the fp64-evaluated totals",
          pybind11::arg("X"), pybind11::arg("W"), pybind11::arg("b"),
          pybind11::arg("col_group"), pybind11::arg("vidx"),
          pybind11::arg("bgp"), pybind11::arg("lfnull64"),
          pybind11::arg("diff"), pybind11::arg("total"), pybind11::arg("act"),
          pybind11::arg("link"));
    m.def("fused_predict_linear_packed", &fused_predict_linear_packed,
          "MFMA fused predict from packed mask words with the link fused into "
          "the epilogue (K3p); mma: -1 auto, 0 fp32 MFMA, 1 split-operand bf16 "
          "MFMA (Mpad <= 12, act 1/3; other shapes take the fp32 MFMA path)",
          pybind11::arg("packed"), pybind11::arg("diff"), pybind11::arg("base"),
          pybind11::arg("wbg"), pybind11::arg("ey"), pybind11::arg("act"),
          pybind11::arg("link") = 0, pybind11::arg("lfnull") = pybind11::none(),
          pybind11::arg("mma") = -1);
    m.def("wls_solve_packed", &wls_solve_packed,
          "MFMA WLS solve with (S,) kernel weights, scattered into "
          "phi_full (B,G,n_out) through vidx (K7p)",
          pybind11::arg("packed"), pybind11::arg("kw"), pybind11::arg("ey_adj"),
          pybind11::arg("total"), pybind11::arg("vidx"),
          pybind11::arg("phi_full"));
    m.def("varying_probe", &varying_probe,
          "varying-pattern probe (K1p): per-instance group bit keys and "
          "[all(keys == keys[0]), keys[0]] in two launches, no host sync",
          pybind11::arg("X"), pybind11::arg("bg_min"), pybind11::arg("bg_max"),
          pybind11::arg("tol_min"), pybind11::arg("tol_max"),
          pybind11::arg("col_group"), pybind11::arg("n_groups"),
          pybind11::arg("keys"), pybind11::arg("probe"));
    m.def("fill_random_masks", &fill_random_masks,
          "Philox coalition sampling (K2)");
    m.def("fused_predict_linear", &fused_predict_linear,
          "MFMA fused mask@diff GEMM + activation + background reduce (K3-K6)");
    m.def("fused_predict_linear_wide", &fused_predict_linear_wide,
          "Column-tile-streamed fused linear predict for 3..16 outputs (K4l)");
    m.def("build_diff_f32", &build_diff_f32,
          "diff image in the f32 fused-kernel layout");
    m.def("build_diff_bf16", &build_diff_bf16,
          "hi(+lo) diff images in the bf16 fused-kernel layout");
    m.def("pack_masks", &pack_masks,
          "masks u8 -> packed u64 bits (for the MFMA WLS Gram build)");
    m.def("fused_predict_bf16", &fused_predict_bf16,
          "bf16 matrix-core fused predict (single or hi+lo split), A-operand "
          "converted in-register from the raw u8 masks");
    m.def("synth_chunk", &synth_chunk,
          "masked-background perturbation synthesis tile (K3')");
    m.def("wls_solve", &wls_solve,
          "batched constrained WLS Shapley solve (K7)",
          pybind11::arg("masks"), pybind11::arg("kw"), pybind11::arg("ey_adj"),
          pybind11::arg("total"), pybind11::arg("phi"),
          pybind11::arg("packed") = pybind11::none());
    m.def("pack_masks_words", &pack_masks_words,
          "masks u8 -> (B,S,W) packed u64 words (wide-M Gram build)");
    m.def("wls_gram", &wls_gram,
          "tiled MFMA Gram+rhs build (fp64 via chunked promotion) for the "
          "stress WLS shapes, M up to 513");
    m.def("fused_predict_tiled", &fused_predict_tiled,
          "tiled MFMA fused predict for Mpad>64 / Npad>128 (LDS-streamed "
          "diff chunks, per-column-tile partials + deterministic reduce)");
    m.def("build_diff_bf16_tiled", &build_diff_bf16_tiled,
          "hi(+lo) k-contiguous diff image for the bf16 tiled predict");
    m.def("fused_predict_tiled_bf16", &fused_predict_tiled_bf16,
          "bf16 matrix-core tiled fused predict (v_mfma_f32_16x16x32_bf16 "
          "per 32-deep k block; hi+lo split for fp32-grade)");
}
