// One cursor lays out every caller-provided workspace.  An op writes its layout once, as a struct of typed pointers
// whose constructor takes the segments from a Carve: over a null base the cursor only counts (*_workspace_bytes), over
// the caller's pointer it hands out what the launches use -- the size and the pointers cannot disagree.
#pragma once
#include <stddef.h>

struct Carve {
  char *base;  // nullptr: count only
  size_t off = 0;
  explicit Carve(void *workspace) : base(static_cast<char *>(workspace)) {}
  // `count` elements of T at the cursor; then the cursor is rounded up to `align` bytes (a power of two)
  template <typename T>
  T *take(size_t count, size_t align = 1) {
    T *p = base ? reinterpret_cast<T *>(base + off) : nullptr;
    off += sizeof(T) * count;
    pad(align);
    return p;
  }
  void pad(size_t align) { off = (off + align - 1) & ~(align - 1); }
  size_t bytes() const { return off; }
};

// the size of layout W for a shape: W's constructor run over a counting cursor
template <typename W, typename... Shape>
size_t carve_bytes(Shape... shape) {
  Carve c(nullptr);
  W w(c, shape...);
  (void)w;
  return c.bytes();
}
