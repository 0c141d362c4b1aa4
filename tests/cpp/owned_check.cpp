// owned_check.cpp -- the owning templates of tools_amd/csrc/psf_owned.hpp (no HIP in them) over a fake acquire / release pair that numbers every handle
// it gives out and records every release: each handle acquired is released exactly once, and in the documented order.  Built with
// -fsanitize=address,undefined (tests/test_cpp_mirror.py); the fake arrays are real heap blocks, so a double release or a leak is also the sanitizer's.
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>
#include "../../tools_amd/csrc/psf_owned.hpp"

static std::vector<void*> g_acquired, g_released;      // in call order
static bool g_fail_next = false;
static size_t g_release_calls = 0;

static int fake_acquire(void** p, size_t bytes) {
  if (g_fail_next) { g_fail_next = false; return 2; }
  *p = std::malloc(bytes ? bytes : 1);
  g_acquired.push_back(*p);
  return 0;
}
static void fake_release(void* p) { ++g_release_calls; g_released.push_back(p); std::free(p); }

// a second kind of handle (what a stream or an event is): small integers behind a pointer type, created by a function that writes the handle
struct Tok; using tok_t = Tok*;
static std::vector<tok_t> g_tok_released;
static long g_tok_next = 1;
static int tok_create(tok_t* out) { *out = reinterpret_cast<tok_t>(g_tok_next++ << 4); return 0; }
static int tok_destroy(tok_t t) { g_tok_released.push_back(t); return 0; }

using Arr = psf::OwnedArr<long, fake_acquire, fake_release>;
using Tk = psf::Owned<tok_t, tok_destroy>;

static int g_bad = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_bad; } } while (0)

static void expect_released(std::vector<void*> want) {      // exactly these, in this order, since the last call
  CHECK(g_released == want);
  g_released.clear();
}

int main() {
  {  // default construction, destruction of an empty object: nothing acquired, nothing released
    Arr a;
    CHECK(a.get() == nullptr && a.cap() == 0 && !a);
    Tk t;
    CHECK(t.get() == nullptr && !t);
  }
  CHECK(g_acquired.empty());
  expect_released({});
  CHECK(g_tok_released.empty());

  {  // alloc, alloc over a held resource (the old one goes first), reset, destruction after reset
    Arr a;
    CHECK(a.alloc(5) == 0 && a.cap() == 5 && a.get() == g_acquired[0]);
    a[4] = 7;                                                // the whole count is there (ASan)
    long* raw = a;                                           // the implicit conversion
    CHECK(raw == a.get() && *(a + 4) == 7 && a);
    CHECK(a.alloc(3, 16) == 0 && a.cap() == 3);
    expect_released({g_acquired[0]});
    reinterpret_cast<char*>(a.get())[3 * sizeof(long) + 15] = 1;      // the slack bytes are there
    a.reset();
    CHECK(a.get() == nullptr && a.cap() == 0);
    expect_released({g_acquired[1]});
    a.reset();                                               // twice: nothing
  }
  expect_released({});

  {  // a failing alloc leaves the object empty and the capacity 0, whatever it held; the next one starts over
    Arr a;
    CHECK(a.alloc(4) == 0);
    g_fail_next = true;
    CHECK(a.alloc(8) == 2 && a.get() == nullptr && a.cap() == 0);
    expect_released({g_acquired[2]});
    g_fail_next = true;
    CHECK(a.grow(8) == 2 && a.get() == nullptr && a.cap() == 0);
    CHECK(a.grow(8) == 0 && a.cap() == 8);
  }
  expect_released({g_acquired[3]});

  {  // growth below, at and above the capacity: kept, kept, released and allocated anew
    Arr a;
    CHECK(a.grow(0) == 0 && a.get() == nullptr);             // nothing asked for: nothing acquired
    CHECK(a.grow(10) == 0 && a.cap() == 10);
    long* const first = a;
    CHECK(a.grow(9) == 0 && a.get() == first && a.cap() == 10);
    CHECK(a.grow(10) == 0 && a.get() == first && a.cap() == 10);
    expect_released({});
    CHECK(a.grow(11, 8) == 0 && a.cap() == 11 && a.get() == g_acquired[5]);
    expect_released({first});
  }
  expect_released({g_acquired[5]});

  {  // move construction, move assignment onto a held resource, self-move-assignment
    Arr a;
    CHECK(a.alloc(2) == 0);
    void* const pa = a.get();
    Arr b(std::move(a));
    CHECK(a.get() == nullptr && a.cap() == 0 && b.get() == pa && b.cap() == 2);
    Arr c;
    CHECK(c.alloc(6) == 0);
    void* const pc = c.get();
    c = std::move(b);                                        // what c held is released, what b held moves
    CHECK(c.get() == pa && c.cap() == 2 && b.get() == nullptr && b.cap() == 0);
    expect_released({pc});
    Arr& alias = c;
    c = std::move(alias);                                    // self: kept
    CHECK(c.get() == pa && c.cap() == 2);
    expect_released({});
    c = Arr{};                                               // how a handle drops a group of buffers: assignment from an empty one
    expect_released({pa});
  }
  expect_released({});

  {  // an array of owners destroyed together: elements in reverse order, each once; a struct's members likewise, after its destructor's body
    struct Group { Arr x[3]; Arr y; std::vector<void*>* seen; ~Group() { seen->assign(g_released.begin(), g_released.end()); } };
    std::vector<void*> at_body;
    void* p[4];
    {
      Group g;
      g.seen = &at_body;
      for (int i = 0; i < 3; ++i) { CHECK(g.x[i].alloc(1 + i) == 0); p[i] = g.x[i].get(); }
      CHECK(g.y.alloc(1) == 0); p[3] = g.y.get();
    }
    CHECK(at_body.empty());                                  // nothing was released before the body ran
    expect_released({p[3], p[2], p[1], p[0]});
  }

  {  // the single-handle owner: put() in front of a create call, reset(h), detach, moves
    Tk t;
    CHECK(tok_create(t.put()) == 0 && t);
    const tok_t first = t;
    CHECK(tok_create(t.put()) == 0);                         // put() releases what was held before the create call writes
    CHECK(g_tok_released == std::vector<tok_t>{first});
    const tok_t second = t;
    Tk u(std::move(t));
    CHECK(!t && u.get() == second);
    Tk v;
    CHECK(tok_create(v.put()) == 0);
    const tok_t third = v;
    v = std::move(u);
    CHECK((g_tok_released == std::vector<tok_t>{first, third}) && v.get() == second && !u);
    Tk& alias = v;
    v = std::move(alias);
    CHECK(v.get() == second);
    CHECK(v.detach() == second && !v);                       // given up, not released
    CHECK((g_tok_released == std::vector<tok_t>{first, third}));
    v.reset(second);                                         // held again
    Tk w[2];
    CHECK(tok_create(w[0].put()) == 0 && tok_create(w[1].put()) == 0);
    g_tok_released.clear();
    const tok_t w0 = w[0], w1 = w[1];
    {
      Tk x[2] = {std::move(w[0]), std::move(w[1])};
    }
    CHECK((g_tok_released == std::vector<tok_t>{w1, w0}));
    g_tok_released.clear();
  }
  CHECK(g_tok_released.size() == 1);                         // v's `second`; t, u, w[] were empty

  // every array acquired over the whole run was released, and no release happened twice (the cases above checked which and when)
  CHECK(g_acquired.size() == 12 && g_release_calls == g_acquired.size());
  if (g_bad) { std::printf("OWNED_CHECK_FAILED %d\n", g_bad); return 1; }
  std::printf("OWNED_OK %zu arrays\n", g_acquired.size());
  return 0;
}
