/*
 * spmv_hip_compact_device.h -- the plan of spmv_hip_compact.h made from DEVICE arrays, and read back.  A matrix that was born on
 * the device (the coarse matrices of spmv_hip_agg.h) gets its compact plan without its columns visiting the host.  Same
 * conventions as spmv_hip.h; callers detect the feature by the presence of the symbols.
 */
#ifndef SPMV_HIP_COMPACT_DEVICE_H
#define SPMV_HIP_COMPACT_DEVICE_H

#include "spmv_hip_compact.h"

#ifdef __cplusplus
extern "C" {
#endif

/* spmv_hip_c16_plan_csr from DEVICE row_ptr (rows + 1 entries) and columns: the same plan bit for bit -- descriptors, bases,
 * codes and every number of spmv_hip_c16_plan_info -- for every multiply that takes a spmv_hip_c16_plan.  Both arrays are read
 * on `stream`, in stream order behind whatever wrote them.  row_ptr (4 bytes per row) is copied to the host, where the tiles are
 * cut; the columns stay on the device: a wave per tile chooses the window bases, one int per tile comes back, the descriptors
 * go up, and a second kernel writes the codes.  No array with an element per stored entry crosses the bus.  The call
 * synchronises `stream`, allocates the plan's device block and frees every temporary; it cannot be captured into a graph.
 * Refused before anything touches the device (*plan is not written): SPMV_HIP_ERR_INVALID for a null plan, rows < 0, cols < 0,
 * a flag other than SPMV_HIP_FLAG_EXACT_ORDER or a null d_row_ptr; SPMV_HIP_ERR_ALIGN for either array off its 4-byte
 * alignment.  Refused after row_ptr was read: what spmv_hip_c16_plan_csr refuses of a row_ptr; SPMV_HIP_ERR_INVALID for a null
 * d_column_index where there are stored entries, and for columns outside [0, cols), which are counted on the device (the
 * message gives the count) and are never used as an address.  A refused call leaves *plan as it was and no device memory
 * behind. */
int spmv_hip_c16_plan_csr_device(spmv_hip_c16_plan **plan, int32_t rows, int32_t cols, const int32_t *d_row_ptr,
                                 const int32_t *d_column_index, unsigned flags, void *stream);

/* A plan, host-made or device-made, read back to HOST arrays in the format of spmv_hip_c16_plan_preview: tile_table, where not
 * null, receives SPMV_HIP_C16_TILE_INTS int32 per tile in launch order (tile_table_ints values of room; ask
 * spmv_hip_c16_plan_info [5]); codes, where not null, the code of every stored entry by entry index, 0 in wide tiles (codes_len
 * values of room; ask [2]).  Too little room, a negative count or a null plan is SPMV_HIP_ERR_INVALID.  Synchronises
 * `stream`. */
int spmv_hip_c16_plan_table(const spmv_hip_c16_plan *plan, int32_t *tile_table, int64_t tile_table_ints, uint16_t *codes,
                            int64_t codes_len, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* SPMV_HIP_COMPACT_DEVICE_H */
