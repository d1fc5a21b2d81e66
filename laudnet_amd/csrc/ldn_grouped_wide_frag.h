// The pre-split weight fragments of the grouped 3x3 at group widths 56 and 112 (ops.pack_grouped_wide_weights; the index formula is in
// include/ldn_hip.h): bf16 [C / gw][NSTEP][MT][64 lanes][8 hi | 8 lo].  The out channels of a group are padded to MT row tiles of 32; K = 9 gw is
// cut into octets, two per K step (width 56: 63 octets in 32 steps, octet 63 a zero pad; width 112: 126 in 63).  One packed copy serves the image
// kernel (ldn_grouped_wide.hip) and the row kernel (ldn_grouped_wide_rows.hip): the geometry is stated here, once.
#pragma once
#include <stddef.h>

namespace ldn {

template <int GW> struct GwCfg;
template <> struct GwCfg<56> { static constexpr int MT = 2, NSTEP = 32; };
template <> struct GwCfg<112> { static constexpr int MT = 4, NSTEP = 63; };
template <int GW> constexpr size_t gw_frag_bytes() { return (size_t)GwCfg<GW>::NSTEP * GwCfg<GW>::MT * 64 * 32; }      // per group

// the same for a run-time width on the host
constexpr bool gw_frag_width(int gw) { return gw == 56 || gw == 112; }
constexpr int gw_frag_mt(int gw) { return gw == 56 ? GwCfg<56>::MT : GwCfg<112>::MT; }
constexpr size_t gw_frag_bytes(int gw) { return gw == 56 ? gw_frag_bytes<56>() : gw_frag_bytes<112>(); }

}  // namespace ldn
