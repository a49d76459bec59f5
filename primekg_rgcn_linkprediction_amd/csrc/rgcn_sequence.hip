// rgcn_sequence_run: a recorded, FIXED list of this library's launches issued by one C call.
//
// The reference runs its layer from Python (src/models/rgcn.py:123,128, once per 1,024-edge batch:
// src/train.py:291-297); so does this package - but on a static graph the launches of one pass are the same list
// every step, only the addresses of the step's tensors change.  The host side (ops.Region) records that list once
// (which entry point, which arguments), classifies every pointer argument as constant (graph structures, handles)
// or as base + offset into one of the step's buffers (the pass's arena, its inputs), and from then on issues the
// whole pass with ONE call into this function: ~14 ctypes calls, their argument checks and a dozen allocations
// become one call and one allocation (host time per eager encoder step: DESIGN.md section 7).
// Nothing here computes: every entry of the table below forwards to the entry point of include/rgcn_hip.h it names
// (rgcn_sequence.h: argument count and conversions come from that entry point's own prototype).
#include "rgcn_sequence.h"

namespace {

const rgcn_seq::entry kTable[] = {                   // in RGCN_FN_* order
    RGCN_SEQ_ENTRY(rgcn_absmax),
    RGCN_SEQ_ENTRY(rgcn_absmax_multi),
    RGCN_SEQ_ENTRY(rgcn_absmax_pack),
    RGCN_SEQ_ENTRY(rgcn_weights_split_pack_multi),
    RGCN_SEQ_ENTRY(rgcn_aggregate),
    RGCN_SEQ_ENTRY(rgcn_aggregate_ex),
    RGCN_SEQ_ENTRY(rgcn_transform_fwd_split),
    RGCN_SEQ_ENTRY(rgcn_transform_bwd_input_split),
    RGCN_SEQ_ENTRY(rgcn_transform_first_split),
    RGCN_SEQ_ENTRY(rgcn_transform_bwd_params_split_begin),
    RGCN_SEQ_ENTRY(rgcn_slab_reduce),
    RGCN_SEQ_ENTRY(rgcn_layer_fwd_fused),
    RGCN_SEQ_ENTRY(rgcn_layer_bwd_input_fused),
    RGCN_SEQ_ENTRY(rgcn_transform_bwd_input_chain_split),
};
static_assert(sizeof(kTable) / sizeof(kTable[0]) == RGCN_FN_COUNT, "one entry per RGCN_FN_*");

}  // namespace

extern "C" int rgcn_sequence_run(const rgcn_seq_call* calls, int num_calls, const rgcn_seq_arg* args, int64_t num_args,
                                 void* const* bases, int num_bases, void* stream) {
  return rgcn_seq::rgcn_sequence_run_table(kTable, calls, num_calls, args, num_args, bases, num_bases, stream);
}
