/* lbl_amd_kdist.h: the weighted band k-distribution entry of liblbl_amd.so, beside lbl_amd.h. */
#ifndef LBL_AMD_KDIST_H_
#define LBL_AMD_KDIST_H_

#include "lbl_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Weighted band k-distributions (Spectroscopy.compute_kdistribution with weighting=): what
 * lbl_band_distribution does, with the permutation kept and a weight per column carried through
 * it -- the Planck fractions and Planck-weighted means of k that a correlated-k table stores
 * beside k(g) (kernels: pylbl_amd/csrc/band_sort_pairs.h).  This entry extends the C ABI of
 * lbl_amd.h, which this header includes and leaves as it is; it is exported by the same library
 * and takes the same engine, grid handles, flags and status codes.
 *
 * values, row_stride, columns, n_rows, band_start, n_bands, scratch, interval_start, n_intervals,
 * means, point_index, point_fraction, n_points, quantiles and flags (LBL_ASYNC or 0) as for
 * lbl_band_distribution; the sorted values, the means and the quantiles are its bit for bit.  A
 * band holds at most 2^31 - 1 columns.
 * Per row and band of N columns, with key() that entry's integer key and j the column's offset
 * from the band's first column, pi is the permutation that sorts the pairs (key(k_j), j)
 * lexicographically: numpy.argsort(keys, kind="stable"), unique, the same for every run cut,
 * layout and repeated call.  With a weight w_j >= 0 per column:
 *   W_i = w_pi(i) ; WK_i = W_i*k_i        (k_i the sorted values; one rounding, no fused
 *                                          multiply-add)
 * The weights: exactly one of
 *   row_temperature (host, [n_rows], finite and > 0): w_j = B(nu_j, T_row), B as in
 *     lbl_path_radiance (0 for nu <= 0) and nu the points of `grid`, a handle of lbl_grid_load
 *     with at least `columns` points (read with row_temperature only);
 *   weight_row (device, [columns]): w_j itself, the same for every row (not checked: the caller
 *     passes finite weights >= 0).
 * Blocks (device):
 *   index_rows (int32, [n_rows][index_stride], index_stride >= columns; required): pi(i) at
 *     column band start + i; columns of no band are not written;
 *   index_scratch (int32, shaped like index_rows) and scratch: needed when a band is longer than
 *     4096 columns; keys and offsets move between the two pairs of blocks together and both
 *     results end in values / index_rows;
 *   weight_rows and weighted_rows ([n_rows][row_stride], NULL: not wanted, both or neither): W
 *     and WK at column band start + i; columns of no band are not written.
 * No two of values, scratch, weight_rows, weighted_rows, weight_row, index_rows and index_scratch
 * may overlap.
 * Outputs per interval (device, [n_rows][n_intervals], NULL: not wanted; they need weight_rows and
 * weighted_rows): weight_sums = the sum of W and weighted_sums = the sum of WK over the columns
 * [interval_start[q], interval_start[q + 1]), added in the fixed order of lbl_path_compute's band
 * means (a partial sum per segment of 4096 columns, the partials in segment order; no atomics,
 * the same bits for every launch shape); 0 for an interval without columns.  n_intervals > 0 goes
 * together with at least one of means, weight_sums and weighted_sums.  The fractions
 * weight_sums/sum of the band's weight_sums and the weighted means weighted_sums/weight_sums are
 * left to the caller.
 * LBL_BAD_ARGUMENT for bad shapes or bands, values or index_rows NULL, both or neither of
 * row_temperature and weight_row, an unknown grid or one with fewer than `columns` points, a row
 * temperature that is not finite and > 0, index_stride < columns, one of weight_rows and
 * weighted_rows without the other, sums without those rows, intervals without an output or an
 * output without intervals, quantiles without their tables, a band longer than 4096 columns without
 * scratch and index_scratch, blocks that overlap, or other flags; nothing is launched and the
 * engine stays usable. */
int lbl_band_distribution_weighted(lbl_engine *engine, double *values, int64_t row_stride,
                                   int64_t columns, int32_t n_rows, const int64_t *band_start,
                                   int32_t n_bands, double *scratch, int32_t grid,
                                   const double *row_temperature, const double *weight_row,
                                   int32_t *index_rows, int32_t *index_scratch,
                                   int64_t index_stride, double *weight_rows,
                                   double *weighted_rows, const int64_t *interval_start,
                                   int32_t n_intervals, double *weight_sums, double *weighted_sums,
                                   double *means, const int64_t *point_index,
                                   const double *point_fraction, int32_t n_points,
                                   double *quantiles, int32_t flags);

#ifdef __cplusplus
}
#endif
#endif
