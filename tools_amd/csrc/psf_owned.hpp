// psf_owned.hpp -- move-only owners of one resource, over the functions that acquire and release it.  No HIP here: psf_hip_util.hpp names the four kinds the library
// holds (device arrays, pinned arrays, streams, events), tests/cpp/owned_check.cpp the same templates over counting fakes.
// Both convert implicitly to the raw handle, so a launch, a copy, `p + off` and `if (p)` read an owner as they read a pointer.
#pragma once
#include <cstddef>
#include <utility>

namespace psf {

// one handle H (a pointer, a stream, an event; H() = none): Release(h) once per handle held, on reset, assignment and destruction
template <class H, auto Release> class Owned {
 public:
  Owned() = default;
  Owned(Owned&& o) noexcept : h_(o.detach()) {}
  Owned& operator=(Owned&& o) noexcept { if (this != &o) reset(o.detach()); return *this; }
  Owned(const Owned&) = delete;
  Owned& operator=(const Owned&) = delete;
  ~Owned() { reset(); }
  void reset(H h = H()) { if (h_) (void)Release(h_); h_ = h; }      // releases what is held, then holds h
  H detach() { H h = h_; h_ = H(); return h; }                       // gives up what is held without releasing it
  H* put() { reset(); return &h_; }                                  // for a create call that writes the handle: hipEventCreate(ev.put())
  H get() const { return h_; }
  operator H() const { return h_; }

 private:
  H h_ = H();
};

// `count` elements of T (+ slack_bytes) from Acquire(void**, bytes), which returns 0 on success.  The operations return Acquire's code (for HIP_TRY).
template <class T, auto Acquire, auto Release> class OwnedArr {
 public:
  OwnedArr() = default;
  OwnedArr(OwnedArr&& o) noexcept : p_(std::move(o.p_)), cap_(o.cap_) { o.cap_ = 0; }
  OwnedArr& operator=(OwnedArr&& o) noexcept { if (this != &o) { p_ = std::move(o.p_); cap_ = o.cap_; o.cap_ = 0; } return *this; }
  // releases what is held first; after a failure the array is empty and its capacity 0
  auto alloc(size_t count, size_t slack_bytes = 0) {
    reset();
    void* v = nullptr;
    const auto e = Acquire(&v, count * sizeof(T) + slack_bytes);
    if (e == decltype(e)()) { p_.reset(static_cast<T*>(v)); cap_ = count; }
    return e;
  }
  // a cached array of at least `need` elements: kept when large enough, else released and allocated anew (the contents are not carried over)
  auto grow(size_t need, size_t slack_bytes = 0) { return need <= cap_ ? decltype(alloc(need))() : alloc(need, slack_bytes); }
  void reset() { p_.reset(); cap_ = 0; }
  size_t cap() const { return cap_; }                                // elements asked for by the last successful alloc / grow
  T* get() const { return p_.get(); }
  operator T*() const { return p_.get(); }

 private:
  Owned<T*, Release> p_;
  size_t cap_ = 0;
};

}  // namespace psf
