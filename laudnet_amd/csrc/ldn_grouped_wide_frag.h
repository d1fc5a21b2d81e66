// The pre-split weight fragments of the grouped 3x3 at group widths 56, 112 and 232 (ops.pack_grouped_wide_weights; the index formula is in
// include/ldn_hip.h): bf16 [C / gw][NSTEP][MT][64 lanes][8 hi | 8 lo].  The out channels of a group are padded to MT row tiles of 32; K = 9 gw is
// cut into octets, two per K step (width 56: 63 octets in 32 steps, octet 63 a zero pad; width 112: 126 in 63; width 232: 261 in 131, octet 261
// a zero pad, and out channels 232-255 of the eighth row tile zero rows).  One packed copy serves the image kernel (ldn_grouped_wide.hip) and
// the row kernel (ldn_grouped_wide_rows.hip): the geometry is stated here, once.
#pragma once
#include <stddef.h>

namespace ldn {

template <int GW> struct GwCfg;
template <> struct GwCfg<56> { static constexpr int MT = 2, NSTEP = 32; };
template <> struct GwCfg<112> { static constexpr int MT = 4, NSTEP = 63; };
template <> struct GwCfg<232> { static constexpr int MT = 8, NSTEP = 131; };
template <int GW> constexpr size_t gw_frag_bytes() { return (size_t)GwCfg<GW>::NSTEP * GwCfg<GW>::MT * 64 * 32; }      // per group
// the last K step's second octet lies past tap 8: a zero pad of the fragments (widths 56 and 232)
template <int GW> constexpr bool gw_frag_pad_octet() { return 2 * GwCfg<GW>::NSTEP > 9 * (GW / 8); }

// the same for a run-time width on the host
constexpr bool gw_frag_width(int gw) { return gw == 56 || gw == 112 || gw == 232; }
constexpr int gw_frag_mt(int gw) { return gw == 56 ? GwCfg<56>::MT : gw == 112 ? GwCfg<112>::MT : GwCfg<232>::MT; }
constexpr size_t gw_frag_bytes(int gw) { return gw == 56 ? gw_frag_bytes<56>() : gw == 112 ? gw_frag_bytes<112>() : gw_frag_bytes<232>(); }

}  // namespace ldn
