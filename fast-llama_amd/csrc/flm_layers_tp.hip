// flm_layers_tp.hip -- host side of the RANK-SPANNING k_layers (flm_layer.h: k_layers<.., TP>; round 6): all layers of a SHARDED token in one launch per rank.
// A translation unit of its own: the instantiations compile beside flm_layers.hip's (same FLM_OPAQUE_TID build, see there).
#define FLM_OPAQUE_TID 1
#include "flm_host.h"

namespace fh {

// the TP instantiations: all-to-all hand-offs (R5 = 0), no tail; [QT][XR2 = 1 | 3][SPLIT][granules | flag rounds: two instantiations -- both forms in one rank-spanning kernel spill]
using VLayersTp = cross_t<VQuant, cross_t<VRounds, cross_t<Variants<Variant<0>, Variant<1>>, Variants<Variant<0>, Variant<1>>>>>;
int launch_layers_tp(flm_ctx* c, hipStream_t st, const LayerArgs* LA, const BackArgs& p, int grid, int r2, int l0, int l1, int G) {
    auto kernel_of = [](auto v) { using V = decltype(v); return &k_layers<V::v[0], V::v[1], V::v[2] != 0, 0, false, true, V::v[3] != 0>; };
    int r = raise_lds_limit<VLayersTp>(c, kernel_of); if (r) return r;
    const int want[] = {quant_variant(c->d.quant_type), rounds_class(r2), G > 1, p.gr != 0};
    if (!dispatch(VLayersTp{}, want, [&](auto v) { hipLaunchKernelGGL(kernel_of(v), dim3(grid), dim3(kGemvBlock), kLdsMax, st, LA, p, l0, l1, (const TailArgs*)nullptr); })) return FLM_ERR_UNSUPPORTED;
    HIPC(c, hipGetLastError());
    return FLM_OK;
}

} // namespace fh
