// nc_ws.h — the one description of a caller-allocated workspace (host only, no HIP include).
// A stage writes one carve function that takes a WsCarve and its shape arguments and returns its
// pointer struct.  The size query runs it on a measuring carver (no base), the launcher on the
// caller's pointer, so a section's size is written once.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace nc {

class WsCarve {
 public:
  explicit WsCarve(void* base = nullptr) : base_(static_cast<char*>(base)) {}

  // The next section: `count` elements of T at the next multiple of `align` (a power of two;
  // the base is taken to be aligned), the offset then advanced by the section's bytes rounded
  // up to `align`.  Null when measuring or after a wrap.
  template <class T>
  T* take(size_t count, size_t align = 256) {
    if (count > SIZE_MAX / sizeof(T)) off_ = SIZE_MAX;
    const size_t at = advance(count * sizeof(T), align);
    return base_ && at != SIZE_MAX ? reinterpret_cast<T*>(base_ + at) : nullptr;
  }
  // a reserved or legacy gap; skip(0, align) only rounds the offset up
  void skip(size_t bytes, size_t align = 256) { advance(bytes, align); }

  // end of the last section; SIZE_MAX once a size or the running offset has wrapped size_t
  size_t bytes() const { return off_; }
  // bytes() plus a size query's slack, SIZE_MAX staying SIZE_MAX
  size_t bytes_plus(size_t slack) const { return off_ > SIZE_MAX - slack ? SIZE_MAX : off_ + slack; }

 private:
  static size_t up(size_t n, size_t align) { return n > SIZE_MAX - (align - 1) ? SIZE_MAX : (n + align - 1) & ~(align - 1); }
  // returns the section's offset and moves off_ past it; SIZE_MAX latches
  size_t advance(size_t bytes, size_t align) {
    const size_t at = up(off_, align), len = up(bytes, align);
    off_ = at == SIZE_MAX || len == SIZE_MAX || at > SIZE_MAX - len ? SIZE_MAX : at + len;
    return off_ == SIZE_MAX ? SIZE_MAX : at;
  }

  char* base_;
  size_t off_ = 0;
};

}  // namespace nc
