/*
 * k_volume.h — absorbing glass (include/rpt/rpt.h rpt_set_material_volumes): the one piece of arithmetic of the rule, Beer-Lambert attenuation of a path's
 * throughput over the segment that ends at a Glass surface reached from its inside,
 *     T_c = expr(-(sigma_c * t))      c = x, y, z      (f32 product, then negate; rptm::expr is the deterministic, correctly rounded one of rpt_math.h)
 *     throughput = throughput * T
 * Called by the volumes variant of the surface stage (k_shade.h shade_slot<.., VOLUMES>, instantiated in rpt_volumes.hip only) and, alone, by the test hook
 * rpt_debug_volume_transmit (rpt_debug.hip) on the device and in the host build.  sigma_c == 0 gives expr(-0) = 1 and leaves the channel bit for bit; a
 * product that overflows gives T = +0.  Few lanes reach this line (only hits from inside glass), so expr's f64 core is affordable; a correctly rounded value
 * is what an independent float64 reading can be held to most tightly.
 */
#ifndef RPT_K_VOLUME_H
#define RPT_K_VOLUME_H

#include "k_common.h"

RPT_HD F3 vol_transmit(F3 throughput, F3 sigma, float t) {
    const F3 tr = f3(rptm::expr(-(sigma.x * t)), rptm::expr(-(sigma.y * t)), rptm::expr(-(sigma.z * t)));
    return throughput * tr;
}

#endif /* RPT_K_VOLUME_H */
