// Carver: the layout helper of the host functions that keep their scratch in one buffer (the estimator units through pqa_estim.hpp,
// pqa_dmcsteps.hip).
#pragma once
#include <cstddef>

// Bump carver of a scratch buffer.  A host function states its layout once, as a function that takes its pieces from a Carver; run over
// a null base it only adds up the bytes (size()), run over the buffer it hands out the pointers, so the two cannot disagree.  Every piece
// starts on an 8-byte boundary.
struct Carver {
  char* base;
  size_t off = 0;
  explicit Carver(void* b = nullptr) : base((char*)b) {}
  template <class T>
  T* take(size_t n) {
    T* p = base ? (T*)(base + off) : nullptr;
    off += (n * sizeof(T) + 7) & ~(size_t)7;
    return p;
  }
  size_t size() const { return off; }
};
