/* rgcn_row_order.h - the occupancy order of a bucketed graph's rows (plain C, librgcn_hip.so).
 *
 * The error codes, the ABI version and the conventions are those of rgcn_hip.h.  The split-precision NT transforms
 * skip the k-tiles of a relation that no row of their 64-row tile has; in node order the occupancy is scattered inside
 * each node-type range, so three of four (tile, relation) blocks stay live where half of the (row, relation) segments
 * have an edge.  With RGCN_MODE_ROW_ORDER a workgroup of those launches owns 64 rows of ONE occupancy word instead:
 * the rows grouped by their word (include/rgcn_sparse.h), groups with more relations first, natural order inside a
 * group.  Row order changes no bit of an NT product - every output row is the same k loop over the same operands - so
 * the results are the same bytes at the same addresses; only which workgroup computes a row changes.
 *
 * The order is built once with the graph, on the host, and lives in the device allocation of the occupancy words,
 * behind their 96 pad words (word offsets from the start of that allocation; P = N rounded up to a multiple of 64,
 * every section starts on a 16-byte boundary):
 *
 *   perm       [P]          row at position p (positions past N: a valid row, never stored)
 *   row_words  [P]          the row words in that order (positions past N: 0)
 *   tile_words [P / 32]     the OR of the row words of positions [32 t, 32 t + 32)
 *   fin_ptr    [P / 32 + 1] structures with deferred hub tails (exactly two plan levels): the level-1 items of the
 *   items      [num_items]  positions' 32-row tile t are items[fin_ptr[t] .. fin_ptr[t + 1]) - four words each
 *                           (begin, end, dst, flags), every item once, in plan order inside a tile
 *
 * The natural-order words in front of it are what they were.
 */
#ifndef RGCN_ROW_ORDER_H
#define RGCN_ROW_ORDER_H

#include "rgcn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One more bit of the `int` option word that carries RGCN_MODE_SPARSE_ROWS (`half` of rgcn_transform_fwd_split and
 * rgcn_transform_bwd_input_split, `has_root1` of rgcn_transform_bwd_input_chain_split): `tile_mask` is the occupancy
 * allocation of a structure that carries an order (rgcn_graph_row_order is not NULL) and the launch takes its row
 * tiles in that order.  Two-pass split arithmetic only (not with bit 0 of `half`).  Values 0 - 3 mean what they meant. */
#define RGCN_MODE_ROW_ORDER 4

typedef struct rgcn_row_order_layout {
  int64_t padded_rows;                               /* P */
  int64_t perm, row_words, tile_words, fin_ptr, items;   /* word offsets of the sections */
  int64_t num_items;                                 /* level-1 items regrouped (0: no deferred hub tails) */
  int64_t total_words;                               /* occupancy words and order together */
} rgcn_row_order_layout;

/* Device pointer of `perm` of that direction (padded_rows <- P), owned by the handle; NULL (padded_rows <- 0) when
 * the structure has no occupancy words (R > 32, no rows, direction not built). */
const int32_t* rgcn_graph_row_order(const rgcn_graph* g, int transposed, int64_t* padded_rows);

/* The whole allocation - the occupancy words of rgcn_occupancy_host, then the order - computed on the HOST from a host
 * copy of rowptr [num_rows * num_relations + 1], exactly what the graph builders upload.  Returns its number of words
 * (0 when num_relations > 32 or num_rows == 0: nothing is written; < 0 for bad arguments); `words` (NULL: size query)
 * receives them, `layout` (or NULL) where the sections are.  No device is touched. */
int64_t rgcn_row_order_host(const int32_t* rowptr, int64_t num_rows, int64_t num_relations, uint32_t* words,
                            rgcn_row_order_layout* layout);

#ifdef __cplusplus
}
#endif

#endif /* RGCN_ROW_ORDER_H */
