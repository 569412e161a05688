// tests/cxx/span_overlap_check.cc -- the span helper behind the aliasing rule of include/scl_hip.h (detail/span.hpp) on the
// cases where an interval test goes wrong: spans that touch without sharing a byte, spans that share exactly one, empty spans
// (no rows, no columns, a NULL pointer) laid over a live one, a pitch larger than the row (the gap belongs to the bounding
// span), the permitted exact alias against its near misses (another pointer, another stride, another group), two inputs on one
// buffer, and extents whose product does not fit size_t or runs past the end of the address space: those are reported as
// WRAPPED -- SCL_ERR_BAD_ARG at the boundary -- and never wrap into a small span that overlaps nothing.  Pointers are integers
// here and nothing is dereferenced.  Host only; also built with -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <string>

#include "scl_hip/detail/span.hpp"
using namespace sclhip::alias;

static long g_bad = 0, g_checks = 0;
static void check(bool ok, const char* what) {
  ++g_checks;
  if (!ok) {
    std::printf("MISMATCH %s\n", what);
    ++g_bad;
  }
}
static const void* at(uintptr_t a) { return reinterpret_cast<const void*>(a); }

int main() {
  const uintptr_t B = 0x10000;
  // ---- touching, one byte of overlap, containment -----------------------------------------------------------------------
  {
    const Operand out = vec("out", at(B), 10, 8, true);                       // [B, B + 80)
    check(pair(out, vec("in", at(B + 80), 10, 8, false)) == DISJOINT, "the input starts where the output ends");
    check(pair(out, vec("in", at(B - 80), 10, 8, false)) == DISJOINT, "the input ends where the output starts");
    check(pair(out, vec("in", at(B + 79), 1, 1, false)) == OVERLAP, "one byte shared at the output's end");
    check(pair(out, vec("in", at(B - 1), 2, 1, false)) == OVERLAP, "one byte shared at the output's start");
    check(pair(vec("in", at(B + 79), 1, 1, false), out) == OVERLAP, "the same with the operands exchanged");
    check(pair(out, vec("in", at(B + 8), 1, 8, false)) == OVERLAP, "an input inside the output");
    check(pair(out, vec("in", at(B - 800), 1000, 8, false)) == OVERLAP, "an output inside the input");
    check(pair(out, vec("in", at(B), 10, 8, false)) == OVERLAP, "the exact alias where no group permits it");
    check(pair(vec("a", at(B), 10, 8, false), vec("b", at(B), 10, 8, false)) == DISJOINT, "two inputs on one buffer");
    check(pair(vec("a", at(B), 10, 8, true), vec("b", at(B + 8), 10, 8, true)) == OVERLAP, "two outputs, one element apart");
  }
  // ---- empty operands cover nothing --------------------------------------------------------------------------------------
  {
    const Operand live = vec("live", at(B), 100, 8, true);
    check(pair(live, vec("n0", at(B + 8), 0, 8, true)) == DISJOINT, "n == 0");
    check(pair(live, mat("rows0", at(B + 8), 0, 16, 4, 8, true)) == DISJOINT, "rows == 0");
    check(pair(live, mat("cols0", at(B + 8), 4, 16, 0, 8, true)) == DISJOINT, "cols == 0");
    check(pair(live, vec("null", nullptr, 100, 8, true)) == DISJOINT, "a NULL operand");
    check(pair(vec("n0", at(B), 0, 8, true), vec("n0", at(B), 0, 8, true)) == DISJOINT, "two empty operands on one address");
    size_t bytes = 1;
    check(span_bytes(mat("rows0", at(B), 0, ~(size_t)0, ~(size_t)0, 8, true), &bytes) && bytes == 0,
          "rows == 0 is empty before any product is formed");
    // (rows - 1) * stride with rows == 0 would be (size_t)-1 * stride: never computed
    std::string msg;
    const Operand ops[2] = {live, mat("rows0", at(B), 0, 1 << 20, 1 << 20, 8, false)};
    check(conflict("t", ops, 2, &msg) == DISJOINT && msg.empty(), "conflict() over an empty operand");
  }
  // ---- a pitch larger than the row: the bounding span includes the gaps ----------------------------------------------------
  {
    // 3 rows of 4 elements, 10 apart, 8 bytes each: rows at B, B + 80, B + 160; the span is [B, B + 192)
    const Operand m = mat("m", at(B), 3, 10, 4, 8, true);
    size_t bytes = 0;
    check(span_bytes(m, &bytes) && bytes == (2 * 10 + 4) * 8, "the span of a pitched matrix is (rows - 1) * stride + cols");
    check(pair(m, vec("gap", at(B + 32), 6, 8, false)) == OVERLAP, "an input that sits in the gap after row 0 is inside the span");
    check(pair(m, vec("after", at(B + 192), 6, 8, false)) == DISJOINT, "the tail of the last row's pitch is not part of the span");
    check(pair(m, vec("last", at(B + 191), 1, 1, false)) == OVERLAP, "the last byte of the last row is");
    check(pair(m, mat("row1", at(B + 80), 1, 10, 4, 8, false)) == OVERLAP, "one row into the matrix");
    // one row: the stride does not count (callers pass any value there)
    check(span_bytes(mat("one", at(B), 1, ~(size_t)0, 4, 8, true), &bytes) && bytes == 32, "a one-row matrix ignores its stride");
  }
  // ---- the permitted exact alias and its near misses -------------------------------------------------------------------------
  {
    const Operand dst = mat("dst", at(B), 3, 10, 4, 8, true, 1);
    check(pair(dst, mat("a", at(B), 3, 10, 4, 8, false, 1)) == DISJOINT, "the same pointer, stride and group");
    check(pair(dst, mat("a", at(B), 2, 10, 4, 8, false, 1)) == DISJOINT, "fewer rows at the same pointer and stride");
    check(pair(dst, mat("a", at(B), 3, 12, 4, 8, false, 1)) == OVERLAP, "the same pointer, another stride");
    check(pair(dst, mat("a", at(B + 8), 3, 10, 4, 8, false, 1)) == OVERLAP, "one element in");
    check(pair(dst, mat("a", at(B + 80), 3, 10, 4, 8, false, 1)) == OVERLAP, "one row in");
    check(pair(dst, mat("a", at(B), 3, 10, 4, 8, false, 2)) == OVERLAP, "another group");
    check(pair(dst, mat("a", at(B), 3, 10, 4, 8, false, 0)) == OVERLAP, "no group");
    check(pair(vec("dst", at(B), 7, 8, true, 1), vec("a", at(B), 7, 8, false, 1)) == DISJOINT, "vectors: the same pointer");
    std::string msg;
    const Operand ops[3] = {vec("dst_dev", at(B), 7, 8, true, 1), vec("a_dev", at(B), 7, 8, false, 1), vec("b_dev", at(B + 8), 7, 8, false, 1)};
    check(conflict("ew", ops, 3, &msg) == OVERLAP, "dst == a is fine, b one element in is not");
    check(msg.find("ew: ") == 0 && msg.find("dst_dev") != std::string::npos && msg.find("b_dev") != std::string::npos &&
              msg.find("a_dev") == std::string::npos,
          "the message names the two operands that overlap and the caller");
  }
  // ---- extents that do not fit: reported, not wrapped -----------------------------------------------------------------------
  {
    const size_t BIG = ~(size_t)0;
    size_t bytes = 0;
    check(!span_bytes(vec("v", at(B), BIG / 8 + 1, 8, true), &bytes), "n * 8 wraps to 0");
    check(!span_bytes(vec("v", at(B), BIG / 4, 8, true), &bytes), "n * 8 wraps to a small number");
    check(!span_bytes(mat("m", at(B), 3, BIG / 2 + 1, 4, 8, true), &bytes), "(rows - 1) * stride wraps");
    check(!span_bytes(mat("m", at(B), 2, BIG - 1, 4, 8, true), &bytes), "(rows - 1) * stride + cols wraps");
    check(span_bytes(vec("v", at(B), BIG / 8, 8, true), &bytes) && bytes == BIG / 8 * 8, "the largest extent that fits");
    uintptr_t lo, hi;
    check(!span_of(vec("v", at(BIG - 15), 4, 8, true), &lo, &hi), "ptr + bytes past the end of the address space");
    check(span_of(vec("v", at(BIG - 32), 4, 8, true), &lo, &hi) && hi == BIG, "ptr + bytes up to the last byte");
    // 2^61 + 1 elements of 8 bytes wrap to 8 bytes: as a wrapped span it would miss the input at B + 64
    const Operand wrapped = vec("out_dev", at(B), ((size_t)1 << 61) + 1, 8, true), in = vec("in_dev", at(B + 64), 4, 8, false);
    check(pair(wrapped, in) == WRAPPED, "a wrapped output against an input it really covers");
    std::string msg;
    const Operand ops[2] = {in, wrapped};
    check(conflict("t", ops, 2, &msg) == WRAPPED && msg.find("out_dev") != std::string::npos && msg.find("overflows") != std::string::npos,
          "conflict() names the operand whose extent overflows");
    // .. also when the other operand is empty or far away: the extent is wrong whatever it meets
    const Operand far[2] = {vec("far_dev", at(B << 8), 4, 8, false), wrapped};
    msg.clear();
    check(conflict("t", far, 2, &msg) == WRAPPED, "a wrapped extent is refused even where nothing overlaps");
  }
  std::printf("span_overlap_check: %ld checks, %ld mismatches\n", g_checks, g_bad);
  return g_bad ? 1 : 0;
}
