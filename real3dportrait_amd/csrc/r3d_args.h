// The argument checks that the entry points share, host only: which arrays may not share a byte, the 2^31 limit of a call, the
// workspace, and alignment.  A NULL pointer or a size that must be positive is one line where it stands and has no helper here.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace r3d {

void set_error(const char* fmt, ...);

// p can take n-byte loads (n a power of two); nullptr (an optional operand that is absent) passes
inline bool aligned(const void* p, size_t n) { return ((uintptr_t)p & (n - 1)) == 0; }
inline bool aligned16(const void* p) { return aligned(p, 16); }

// One array of a call: `bytes` bytes at p, written by the call (output) or only read.
struct Span { const void* p; size_t bytes; bool output; };
template <class T> inline Span reads(const T* p, size_t count) { return Span{p, count * sizeof(T), false}; }
template <class T> inline Span writes(const T* p, size_t count) { return Span{p, count * sizeof(T), true}; }

// Do two spans of the list share a byte, at least one of them an output?  A span with a NULL pointer or no bytes takes no part.  The
// distance of the two addresses is compared, never an end p + bytes, so a span at the top of the address space cannot wrap.
inline bool clash(const Span* s, size_t count)
{
    for (size_t i = 0; i < count; ++i)
        for (size_t j = i + 1; j < count; ++j) {
            if (!s[i].p || !s[j].p || !s[i].bytes || !s[j].bytes || !(s[i].output || s[j].output)) continue;
            const uintptr_t a = (uintptr_t)s[i].p, b = (uintptr_t)s[j].p;
            if (a <= b ? b - a < s[i].bytes : a - b < s[j].bytes) return true;
        }
    return false;
}
template <size_t N> inline bool clash(const Span (&s)[N]) { return clash(s, N); }

// the two-span form: [a, a + na) and [b, b + nb) (counts of floats) share an element
inline bool overlap(const float* a, size_t na, const float* b, size_t nb) { const Span s[2] = {writes(a, na), reads(b, nb)}; return clash(s); }

// A call addresses fewer than 2^31 bytes or elements of an array.  `value` is what `expr` ("4 B H W") comes to, counted in `unit`; at
// 2^31 or above the answer is false and the message is `what`'s, or nobody's when `what` is NULL.
inline bool below_2_31(const char* what, const char* expr, double value, const char* unit)
{
    if (value < 2147483648.0) return true;
    if (what) set_error("%s: %s = %.0f %s, the limit per call is 2^31", what, expr, value, unit);
    return false;
}

// The caller's workspace: there, of at least `need` bytes (what `sizer` returns) and `align`-byte aligned; the first miss decides the
// message, and alignment comes before the size where `alignment_first` says so.  The status code is the caller's.
inline bool workspace_ok(const char* what, const void* ws, size_t given, size_t need, size_t align, const char* sizer, bool alignment_first = false)
{
    if (!ws) { set_error("%s: NULL workspace", what); return false; }
    const bool small = given < need, skew = !aligned(ws, align);
    if (skew && (alignment_first || !small)) { set_error("%s: the workspace is not %zu-byte aligned", what, align); return false; }
    if (small) { set_error("%s: the workspace holds %zu bytes, %zu are needed (%s)", what, given, need, sizer); return false; }
    return true;
}

}  // namespace r3d
