// include/scl_hip/detail/span.hpp -- the aliasing rule of include/scl_hip.h (Conventions) as host code.
//
// Every launcher of the core library describes the device operands of its call as a list of Operand and asks conflict() before it
// enqueues anything.  An operand covers its bounding span [ptr, ptr + ((rows - 1) * stride + cols) * elem) -- for a pitched
// matrix that includes the gaps between rows, as in hm_unit.hip.  Two operands of which at least one is written must not share a
// byte, with one exception: operands of the same non-zero `group` may COINCIDE -- the same pointer and, where either has more
// than one row, the same stride -- because the header permits that exact alias for the entry point.  An operand with a NULL
// pointer, no rows or no columns covers nothing.  An extent that does not fit size_t, or that runs past the end of the address
// space, is an error of its own (wrapped): it is reported, never wrapped around.
//
// Host only, no HIP: tests/cxx/span_overlap_check.cc runs it under the host sanitizers.
#ifndef SCL_HIP_DETAIL_SPAN_HPP
#define SCL_HIP_DETAIL_SPAN_HPP

#include <cstddef>
#include <cstdint>
#include <string>

namespace sclhip {
namespace alias {

struct Operand {
  const char* name;  // the parameter's name in include/scl_hip.h
  const void* ptr;
  size_t rows, stride, cols;  // in elements; a vector is one row
  size_t elem;                // bytes per element
  bool written;
  int group;  // operands with the same non-zero group may coincide exactly
};

inline Operand vec(const char* name, const void* p, size_t n, size_t elem, bool written, int group = 0) {
  return Operand{name, p, 1, n, n, elem, written, group};
}
inline Operand mat(const char* name, const void* p, size_t rows, size_t stride, size_t cols, size_t elem, bool written,
                   int group = 0) {
  return Operand{name, p, rows, stride, cols, elem, written, group};
}

enum Verdict { DISJOINT = 0, OVERLAP = 1, WRAPPED = 2 };

inline bool empty(const Operand& o) { return !o.ptr || o.rows == 0 || o.cols == 0 || o.elem == 0; }

// bytes of the bounding span; false if ((rows - 1) * stride + cols) * elem does not fit size_t
inline bool span_bytes(const Operand& o, size_t* bytes) {
  if (empty(o)) {
    *bytes = 0;
    return true;
  }
  size_t e = 0;
  if (__builtin_mul_overflow(o.rows - 1, o.stride, &e)) return false;
  if (__builtin_add_overflow(e, o.cols, &e)) return false;
  return !__builtin_mul_overflow(e, o.elem, bytes);
}

// [lo, hi) as integers; false if the extent wraps size_t or the end of the address space
inline bool span_of(const Operand& o, uintptr_t* lo, uintptr_t* hi) {
  size_t bytes = 0;
  if (!span_bytes(o, &bytes)) return false;
  *lo = reinterpret_cast<uintptr_t>(o.ptr);
  return !__builtin_add_overflow(*lo, (uintptr_t)bytes, hi);
}

inline bool coincide(const Operand& a, const Operand& b) {
  return a.ptr == b.ptr && ((a.rows <= 1 && b.rows <= 1) || a.stride == b.stride);
}

// the verdict on one pair (both spans valid): OVERLAP unless they share no byte or are a permitted exact alias
inline Verdict pair(const Operand& a, const Operand& b) {
  if (empty(a) || empty(b)) return DISJOINT;
  uintptr_t alo, ahi, blo, bhi;
  if (!span_of(a, &alo, &ahi) || !span_of(b, &blo, &bhi)) return WRAPPED;
  if (!(alo < bhi && blo < ahi)) return DISJOINT;
  if (!a.written && !b.written) return DISJOINT;  // two inputs may share memory
  if (a.group && a.group == b.group && coincide(a, b)) return DISJOINT;
  return OVERLAP;
}

// all pairs of ops[0 .. count): the first finding, with both operands named in *msg ("<who>: x overlaps y")
inline Verdict conflict(const char* who, const Operand* ops, size_t count, std::string* msg) {
  for (size_t i = 0; i < count; ++i) {
    uintptr_t lo, hi;
    if (!span_of(ops[i], &lo, &hi)) {
      *msg = std::string(who) + ": the extent of " + ops[i].name + " overflows";
      return WRAPPED;
    }
  }
  for (size_t i = 0; i < count; ++i)
    for (size_t j = i + 1; j < count; ++j)
      if (pair(ops[i], ops[j]) == OVERLAP) {
        const bool exact = ops[i].group && ops[i].group == ops[j].group;
        *msg = std::string(who) + ": " + ops[i].name + " overlaps " + ops[j].name +
               (exact ? " (they may coincide -- the same pointer and stride -- and not overlap otherwise)" : "");
        return OVERLAP;
      }
  return DISJOINT;
}

}  // namespace alias
}  // namespace sclhip
#endif  // SCL_HIP_DETAIL_SPAN_HPP
