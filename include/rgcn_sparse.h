/* rgcn_sparse.h - row-granular relation occupancy of a bucketed graph (plain C, librgcn_hip.so).
 *
 * The error codes, the ABI version and the conventions are those of rgcn_hip.h.  About half of the (node, relation)
 * segments of a typed knowledge graph have no edge.  A training pass neither stores nor reads their rows of an
 * aggregate (RGCN_MODE_SPARSE_ROWS in rgcn_hip.h); what tells a kernel which rows those are is built once with the
 * graph, next to the tile mask and in the same device allocation:
 *
 *   words [0, ceil(N / 32))            rgcn_graph_tile_mask: bit r of word t = some row of [32 t, 32 t + 32) has an
 *                                      edge of relation r
 *   words [row_offset, row_offset + N) bit r of word i = segment (i, r) has an edge; a tile word is the OR of its rows
 *   96 zero words                      the rows a consumer's last tiles reach past N
 *
 * row_offset = ceil(N / 32) rounded up to a multiple of 4 words.  Both directions of a square graph have their own;
 * a structure with more than 32 relations has neither.
 */
#ifndef RGCN_SPARSE_H
#define RGCN_SPARSE_H

#include "rgcn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Device pointer of the row words of that direction (num_rows <- N), owned by the handle; NULL (num_rows <- 0) when
 * the structure has no occupancy words (R > 32, no rows, direction not built). */
const uint32_t* rgcn_graph_row_mask(const rgcn_graph* g, int transposed, int64_t* num_rows);

/* The same words computed on the HOST from a host copy of rowptr [num_rows * num_relations + 1] - what the graph
 * builders upload.  Returns the number of words of the layout above (0 when num_relations > 32: nothing is written,
 * < 0 for bad arguments); `words` (NULL: size query) receives them, `row_offset` (or NULL) where the row words start.
 * No device is touched. */
int64_t rgcn_occupancy_host(const int32_t* rowptr, int64_t num_rows, int64_t num_relations, uint32_t* words,
                            int64_t* row_offset);

#ifdef __cplusplus
}
#endif

#endif /* RGCN_SPARSE_H */
