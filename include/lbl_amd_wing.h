/* lbl_amd_wing.h: the far-wing group records of liblbl_amd.so, beside lbl_amd.h.  For tests. */
#ifndef LBL_AMD_WING_H_
#define LBL_AMD_WING_H_

#include "lbl_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The record the engine keeps per table-aligned eight of far-wing lines and level, from the
 * per-line scalars of the eight (centre = nu + p delta, g2 = gamma^2, bl = S gamma/pi); `lines` of
 * them (0..8) belong to the table.  The same code makes the records of a call, on the host and on
 * the device.  record[26] = eight times (s, nas, gs), then beta and m:
 *   m = rint(centre[0]); beta = the geometric mean of the eight bl;
 *   s = sqrt(beta/bl), nas = -((centre - m) s), gs = g2 (s s) per line.
 * Returns 1 for a scaled group; 0 for a plain one, whose record is (0, 0, 1) eight times, then
 * 0 and 0 (a group that adds 0/1 wherever the record is evaluated): fewer than eight
 * lines, a bl that is not a positive normal number, a centre farther than 1.5 from m, binary
 * exponents of the bl more than 128 apart, or a field that is not finite (s, gs, beta: not
 * normal).  -1 for a null pointer. */
int lbl_wing_group(const double *centre, const double *g2, const double *bl, int32_t lines,
                   double *record);

#ifdef __cplusplus
}
#endif

#endif
