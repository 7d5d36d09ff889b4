// flm_layers.hip -- host side of k_layers (flm_layer.h): ALL layers of a token in one launch.  A translation unit of its own because the kernel is compiled with
// FLM_OPAQUE_TID (flm_math.h: reads of threadIdx.x are opaque, so that nothing derived from it is hoisted out of the loop over layers and kept in registers).
#define FLM_OPAQUE_TID 1
#include "flm_host.h"

namespace fh {

int launch_layers_tp(flm_ctx* c, hipStream_t st, const LayerArgs* LA, const BackArgs& p, int grid, int r2, int l0, int l1, int G);           // flm_layers_tp.hip

// the layers' argument blocks in device memory, per number of workgroups a head is spread over (G = 1 | hs / 32): built outside any stream capture, valid until an option changes
int layers_prepare(flm_ctx* c, int G) {
    const int key = G > 1 ? 1 : 0;
    if (!wants_layers(c) || (c->world != 1 && !(c->p2p && c->grp_tpl))) return FLM_OK;            // (tensor parallel: the rank-spanning form, where the group agreed on it)
    if (c->la_valid[key]) return FLM_OK;
    const int L = c->d.n_layers, qt = c->d.quant_type;
    std::vector<LayerArgs> host((size_t)L);
    c->la_ok[key] = false; c->tail_ok[key] = false;
    const std::string err0 = c->err, gerr0 = g_last_error;
    TailArgs tail{};
    for (int l = 0; l < L; ++l) {
        BackArgs p; int grid = 0, r2 = 0;
        const int r = plan_layer_qt(c, qt, l, true, G, host[l], p, grid, r2, &tail);
        if (r == FLM_ERR_UNSUPPORTED) { c->la_valid[key] = true; c->err = err0; g_last_error = gerr0; return FLM_OK; }      // (this shape runs one launch per layer, or per phase: a probe, not a failure -- flm_last_error keeps what it said)
        if (r) return r;
        c->la_p[key] = p; c->la_grid[key] = grid; c->la_r2[key] = r2;
    }
    HIPC(c, hipMemcpyAsync(c->la_dev[key], host.data(), sizeof(LayerArgs) * (size_t)L, hipMemcpyHostToDevice, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));                                           // (host goes out of scope)
    if (tail.gridc > 0) {   // the one-launch token's argument block (every layer planned with the classifier's layout below the stash: the same st_base throughout)
        HIPC(c, hipMemcpyAsync(c->tail_dev[key], &tail, sizeof(TailArgs), hipMemcpyHostToDevice, c->stream));
        HIPC(c, hipStreamSynchronize(c->stream));
        c->tail_ok[key] = true;
    }
    c->la_ok[key] = true; c->la_valid[key] = true;
    return FLM_OK;
}

// the instantiations of k_layers on one GPU: [QT][XR2][SPLIT][R5 = 0 | 3 (both arrival-order hand-offs)][TAIL]
using VLayers = cross_t<VQuant, cross_t<VRounds, cross_t<Variants<Variant<0>, Variant<1>>, cross_t<Variants<Variant<0>, Variant<3>>, Variants<Variant<0>, Variant<1>>>>>>;
// layers [l0, l1) of the token in one launch; FLM_ERR_UNSUPPORTED: not prepared / not possible for this shape
int launch_layers(flm_ctx* c, hipStream_t st, int l0, int l1, int G, bool tail) {
    const int key = G > 1 ? 1 : 0;
    if (!wants_layers(c) || !c->la_valid[key] || !c->la_ok[key] || l1 <= l0) return FLM_ERR_UNSUPPORTED;
    if (tail && (!c->tail_ok[key] || l0 != 0 || l1 != c->d.n_layers)) return FLM_ERR_UNSUPPORTED;
    if (c->world > 1) {
        if (tail || !c->p2p || !c->grp_tpl || !c->la_p[key].tp.world) return FLM_ERR_UNSUPPORTED;
        return launch_layers_tp(c, st, (const LayerArgs*)c->la_dev[key], c->la_p[key], c->la_grid[key], c->la_r2[key], l0, l1, G);
    }
    auto kernel_of = [](auto v) { using V = decltype(v); return &k_layers<V::v[0], V::v[1], V::v[2] != 0, V::v[3], V::v[4] != 0>; };
    int r = raise_lds_limit<VLayers>(c, kernel_of); if (r) return r;
    BackArgs p = c->la_p[key];
    if (!tail) { p.gr = 0; if (c->back_pre13 == 99) p.pre13 = 16; if (c->tok_preq == 99) p.preq = 16; }                                                                // (granule tags count from the tail launch's epoch: flm_layer.h BackArgs::gr)
    const LayerArgs* LA = (const LayerArgs*)c->la_dev[key];
    const TailArgs* TA = tail ? (const TailArgs*)c->tail_dev[key] : nullptr;
    const int want[] = {quant_variant(c->d.quant_type), rounds_class(c->la_r2[key]), G > 1, p.r5 ? 3 : 0, tail};
    if (!dispatch(VLayers{}, want, [&](auto v) { hipLaunchKernelGGL(kernel_of(v), dim3(c->la_grid[key]), dim3(kGemvBlock), kLdsMax, st, LA, p, l0, l1, TA); })) return FLM_ERR_UNSUPPORTED;
    HIPC(c, hipGetLastError());
    return FLM_OK;
}

} // namespace fh
