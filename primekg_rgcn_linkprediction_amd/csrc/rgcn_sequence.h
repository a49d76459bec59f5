// How rgcn_sequence_run (rgcn_sequence.hip) forwards a recorded call: host-only, nothing of HIP, so a plain C++17
// compiler builds it and tests/seq_forward_check.cpp drives the very loop the library runs over stubs of its own.
// An entry point becomes forwardable by ONE line in a table, RGCN_SEQ_ENTRY(name): its parameter count and the
// conversion of every argument come from its own prototype in include/rgcn_hip.h.
#ifndef RGCN_SEQUENCE_H
#define RGCN_SEQUENCE_H

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <type_traits>
#include <utility>

#include "../../include/rgcn_hip.h"

namespace rgcn_seq {

// A resolved argument is one 64-bit slot.  Floating-point parameters: the bits of a double, narrowed; pointers: the
// address; every other arithmetic parameter: the signed 64-bit value, converted.
template <class T>
inline T from_slot(uint64_t slot) {
  if constexpr (std::is_floating_point_v<T>) {
    double d;
    memcpy(&d, &slot, 8);
    return (T)d;
  } else if constexpr (std::is_pointer_v<T>) {
    return reinterpret_cast<T>(slot);
  } else {
    static_assert(std::is_arithmetic_v<T>, "a forwarded parameter is a number or a pointer");
    return static_cast<T>((int64_t)slot);
  }
}

struct entry {
  int arity;
  int (*run)(const uint64_t* slots);
};

template <auto Fn, class = decltype(Fn)>
struct forward;
template <auto Fn, class... A>
struct forward<Fn, int (*)(A...)> {
  static constexpr int arity = sizeof...(A);
  static_assert(arity <= RGCN_SEQ_MAX_ARGS, "more parameters than a recorded call can carry");
  template <size_t... I>
  static int call(const uint64_t* slots, std::index_sequence<I...>) {
    return Fn(from_slot<A>(slots[I])...);
  }
  static int run(const uint64_t* slots) { return call(slots, std::index_sequence_for<A...>{}); }
};
#define RGCN_SEQ_ENTRY(fn) {rgcn_seq::forward<&fn>::arity, &rgcn_seq::forward<&fn>::run}

// rgcn_sequence_run over `table` (indexed by rgcn_seq_call::fn)
template <size_t N>
int rgcn_sequence_run_table(const entry (&table)[N], const rgcn_seq_call* calls, int num_calls, const rgcn_seq_arg* args,
                            int64_t num_args, void* const* bases, int num_bases, void* stream) {
  if (num_calls < 0 || num_args < 0 || (num_calls > 0 && (!calls || !args)) || num_bases < 0 || (num_bases > 0 && !bases))
    return RGCN_ERR_ARG;
  rgcn_slab_job jobs[RGCN_SEQ_MAX_JOBS];
  for (auto& j : jobs) j = rgcn_slab_job{};
  for (int c = 0; c < num_calls; ++c) {
    const rgcn_seq_call& call = calls[c];
    if (call.num_args < 0 || call.num_args > RGCN_SEQ_MAX_ARGS || call.first_arg < 0 ||
        call.first_arg + call.num_args > num_args)
      return RGCN_ERR_ARG;
    uint64_t slots[RGCN_SEQ_MAX_ARGS];
    uint64_t arrays[RGCN_SEQ_MAX_ARRAYS][RGCN_SEQ_MAX_ARRAY_ENTRIES];
    int used_arrays = 0;
    for (int i = 0; i < call.num_args; ++i) {
      const rgcn_seq_arg& a = args[call.first_arg + i];
      switch (a.kind) {
        case RGCN_SEQ_IMM: slots[i] = (uint64_t)a.value; break;
        case RGCN_SEQ_FLOAT: slots[i] = (uint64_t)a.value; break;                 // the bits of a double
        case RGCN_SEQ_BASE:
          if (a.index < 0 || a.index >= num_bases) return RGCN_ERR_ARG;
          slots[i] = (uint64_t)((char*)bases[a.index] + a.value);
          break;
        case RGCN_SEQ_JOB:
          if (a.index < 0 || a.index >= RGCN_SEQ_MAX_JOBS) return RGCN_ERR_ARG;
          slots[i] = (uint64_t)&jobs[a.index];
          break;
        case RGCN_SEQ_STREAM: slots[i] = (uint64_t)stream; break;
        case RGCN_SEQ_ARRAY: {                       // a HOST array argument: its `value` entries start at args[index]
          if (used_arrays >= RGCN_SEQ_MAX_ARRAYS || a.value < 0 || a.value > RGCN_SEQ_MAX_ARRAY_ENTRIES || a.index < 0 ||
              a.index + a.value > num_args)
            return RGCN_ERR_ARG;
          uint64_t* dst = arrays[used_arrays++];
          for (int64_t k = 0; k < a.value; ++k) {
            const rgcn_seq_arg& e = args[a.index + k];
            if (e.kind == RGCN_SEQ_IMM) dst[k] = (uint64_t)e.value;
            else if (e.kind == RGCN_SEQ_BASE && e.index >= 0 && e.index < num_bases) dst[k] = (uint64_t)((char*)bases[e.index] + e.value);
            else return RGCN_ERR_ARG;
          }
          slots[i] = (uint64_t)dst;
          break;
        }
        default: return RGCN_ERR_ARG;
      }
    }
    if (call.fn < 0 || (size_t)call.fn >= N) return RGCN_ERR_UNSUPPORTED;
    if (call.num_args != table[call.fn].arity) return RGCN_ERR_ARG;
    const int rc = table[call.fn].run(slots);
    if (rc != RGCN_OK) return rc;
  }
  return RGCN_OK;
}

}  // namespace rgcn_seq

#endif  // RGCN_SEQUENCE_H
