// Check of probqa_amd/csrc/c_abi_shims.h -- the exception barrier, the three null-handle conventions of the C ABI and the factory
// helper -- with lambdas in place of engines, no GPU and no HIP library (tests/test_abi_shims.py builds it with g++, plain and with
// -fsanitize=address,undefined).  The engine handle is a dummy that no lambda touches.  Prints "ok <checks>" and exits 0, or names
// the broken property and exits 1.  What the logging shim writes goes to stderr, one line a case; the Python side reads it.
#include <cstdio>
#include <cstdlib>
#include <new>
#include <stdexcept>
#include <string>

#include "../probqa_amd/csrc/c_abi_shims.h"

using namespace pqa;
using namespace pqa::abi;

static int gChecks = 0;
#define CHECK(cond, ...)                                              \
  do {                                                                \
    gChecks++;                                                        \
    if (!(cond)) {                                                    \
      std::fprintf(stderr, "FAILED line %d: %s: ", __LINE__, #cond);  \
      std::fprintf(stderr, __VA_ARGS__);                              \
      std::fprintf(stderr, "\n");                                     \
      std::_Exit(1);                                                  \
    }                                                                 \
  } while (0)

alignas(16) static char gDummy[64];
static void *const kHandle = gDummy;                       // "an engine" / "a factory": never dereferenced
static void *const kStale = gDummy + 32;                   // what *ppError holds before a call: every call must overwrite it
static int gReceived = 0, gReleased = 0;

// The outcomes a callable can have; Throws(c) is what a lambda runs first.
enum Case { Success, ReturnsError, BadAlloc, RuntimeError, Int };
static const Case kCases[] = {Success, ReturnsError, BadAlloc, RuntimeError, Int};
static Error Refusal() { return Error::MakeP(ErrCode::AbsentId, "id=5", "No such quiz."); }
static void Throws(Case c) {
  if (c == BadAlloc) throw std::bad_alloc();
  if (c == RuntimeError) throw std::runtime_error("boom");
  if (c == Int) throw 7;
}

// The error object a case must produce (null for Success), released here as a caller of the C ABI would.
static void ExpectAndRelease(void *pvErr, Case c, const char *shim) {
  if (c == Success) { CHECK(pvErr == nullptr, "%s: an error object on success", shim); return; }
  CHECK(pvErr != nullptr && pvErr != kStale, "%s case %d: no error object", shim, (int)c);
  gReceived++;
  Error *e = static_cast<Error *>(pvErr);
  if (c == ReturnsError) {
    CHECK(e->code == ErrCode::AbsentId && e->message == "No such quiz." && e->hasParams && e->params == "id=5", "%s: the callable's error came back as [%s] [%s]",
          shim, e->message.c_str(), e->params.c_str());
  } else if (c == Int) {
    CHECK(e->code == ErrCode::SRException && e->message == "An unknown exception was caught at the C interface." && !e->hasParams, "%s: throw 7 gave code %d [%s]", shim,
          (int)e->code, e->message.c_str());
  } else {
    const std::string want = c == BadAlloc ? std::string("what=[") + std::bad_alloc().what() + "]" : "what=[boom]";
    CHECK(e->code == ErrCode::StdException && e->message == "A C++ exception was caught at the C interface." && e->hasParams && e->params == want,
          "%s case %d: code %d [%s] [%s]", shim, (int)c, (int)e->code, e->message.c_str(), e->params.c_str());
  }
  delete e;   // CiReleasePqaError
  gReleased++;
}
static void ExpectNullHandle(void *pvErr, const char *what, const char *shim) {
  CHECK(pvErr != nullptr && pvErr != kStale, "%s: no error object for a null handle", shim);
  gReceived++;
  Error *e = static_cast<Error *>(pvErr);
  CHECK(e->code == ErrCode::NullArgument && e->message == std::string("Nullptr is passed in place of ") + what + "." && !e->hasParams, "%s: [%s]", shim, e->message.c_str());
  delete e;
  gReleased++;
}

int main() {
  int calls = 0;
  // ---- returns an error object
  ExpectNullHandle(ErrorOf(nullptr, [&](IEngine &) { calls++; return Error(); }), "IPqaEngine", "ErrorOf");
  CHECK(calls == 0, "ErrorOf ran its callable for a null handle");
  for (Case c : kCases) {
    void *err = ErrorOf(kHandle, [&](IEngine &) { calls++; Throws(c); return c == ReturnsError ? Refusal() : Error(); });
    ExpectAndRelease(err, c, "ErrorOf");
  }
  CHECK(calls == 5, "ErrorOf: %d calls", calls);

  // ---- sets *ppError and returns a value; with every error the fail value; a null ppError is tolerated
  for (int withError = 1; withError >= 0; withError--) {
    void *err = kStale;
    void **ppError = withError ? &err : nullptr;
    calls = 0;
    CHECK(ValueOf<int64_t>(nullptr, ppError, -1, [&](IEngine &, Error &) { calls++; return (int64_t)42; }) == -1 && calls == 0, "ValueOf: a null handle");
    if (withError) ExpectNullHandle(err, "IPqaEngine", "ValueOf");
    for (Case c : kCases) {
      err = kStale;
      const int64_t v = ValueOf<int64_t>(kHandle, ppError, -1, [&](IEngine &, Error &e) {
        calls++;
        Throws(c);
        if (c == ReturnsError) e = Refusal();
        return (int64_t)42;
      });
      CHECK(v == (c == Success ? 42 : -1), "ValueOf case %d returned %lld", (int)c, (long long)v);
      if (withError) ExpectAndRelease(err, c, "ValueOf");
    }
    CHECK(calls == 5, "ValueOf: %d calls", calls);
  }
  CHECK(ValueOf<uint64_t>(kHandle, nullptr, 0, [&](IEngine &, Error &) { return (uint64_t)1 << 40; }) == (uint64_t)1 << 40, "ValueOf<uint64_t>");

  // ---- logs and returns a value: a line on stderr for the null handle and for each exception
  calls = 0;
  CHECK(LoggedOf<uint8_t>(nullptr, 0, [&](IEngine &) { calls++; return true; }) == 0 && calls == 0, "LoggedOf: a null handle");
  for (Case c : kCases) {
    if (c == ReturnsError) continue;   // (these callables have no error to return: a value or an exception)
    const int64_t v = LoggedOf<int64_t>(kHandle, -1, [&](IEngine &) { calls++; Throws(c); return (int64_t)42; });
    CHECK(v == (c == Success ? 42 : -1), "LoggedOf case %d returned %lld", (int)c, (long long)v);
  }
  CHECK(calls == 4, "LoggedOf: %d calls", calls);
  const char *name = LoggedOf<const char *>(kHandle, "", [&](IEngine &) { return "kernel"; });
  CHECK(std::string(name) == "kernel", "LoggedOf<const char *>");
  name = LoggedOf<const char *>(kHandle, "", [&](IEngine &) -> const char * { throw std::runtime_error("name"); });
  CHECK(name != nullptr && *name == 0, "LoggedOf<const char *>: the fail value");

  // ---- the factory's entries
  IEngine *const made = AsEngine(kHandle);
  for (int withError = 1; withError >= 0; withError--) {
    void *err = kStale;
    void **ppError = withError ? &err : nullptr;
    calls = 0;
    CHECK(EngineOf(nullptr, ppError, [&](Error &) { calls++; return made; }) == nullptr && calls == 0, "EngineOf: a null factory");
    if (withError) ExpectNullHandle(err, "IPqaEngineFactory", "EngineOf");
    for (Case c : kCases) {
      err = kStale;
      void *eng = EngineOf(kHandle, ppError, [&](Error &e) -> IEngine * {
        calls++;
        Throws(c);
        if (c == ReturnsError) e = Refusal();
        return c == ReturnsError ? nullptr : made;
      });
      CHECK(eng == (c == Success ? kHandle : nullptr), "EngineOf case %d returned %p", (int)c, eng);
      if (withError) ExpectAndRelease(err, c, "EngineOf");
    }
    CHECK(calls == 5, "EngineOf: %d calls", calls);
  }

  // ---- the barrier alone, as the entries without an engine use it
  for (Case c : kCases) ExpectAndRelease(ReturnErr(Guarded([&] { Throws(c); return c == ReturnsError ? Refusal() : Error(); })), c, "Guarded");
  CHECK(GuardedValue<int64_t>(nullptr, -1, [&](Error &) -> int64_t { throw std::bad_alloc(); }) == -1, "GuardedValue: the fail value");
  CHECK(GuardedValue<char *>(nullptr, nullptr, [&](Error &) -> char * { throw 7; }) == nullptr, "GuardedValue: a null string");

  CHECK(gReceived == gReleased && gReceived == 3 * (1 + 4) + 4,"%d error objects received, %d released", gReceived, gReleased);
  std::printf("ok %d\n", gChecks);
  return 0;
}
