// What more than one part of the string layer (strings*.cpp) uses and strings.h does not show.
#pragma once
#include <vector>

#include "../../include/fhestring_hip.h"
#include "strings.h"

namespace fhs {

inline size_t adjust_end_of_pattern(size_t e) { return e == 0 ? 1 : e; }   // utils.rs:106-112
inline unsigned absent_value(size_t halves) { return halves == 1 ? FHS_MAX_FIND_LENGTH : FHS_WIDE_ABSENT; }
Ref sum_refs(Engine *e, const Ref *r, size_t n);                 // the sum of any number of blocks
void distinct_flags(const Engine *e, std::vector<Ref> &f);       // drops the flags that say what an earlier one says

}  // namespace fhs
