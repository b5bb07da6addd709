// c_abi_shims.h -- what every entry of c_abi.cpp is made of: the exception barrier, and one shim for each of the reference's three
// null-handle conventions (ProbQA/PqaCore/PqaCInterop.cpp:65-86: return an error object, set *ppError, or log and return a value).
// Nothing thrown inside a shim's callable crosses the C ABI: it comes back as an error object with one of the reference's two
// exception codes (its engine methods end in CATCH_TO_ERR_SET / CATCH_TO_ERR_RETURN, ErrorHelper.h).  No engine and no HIP call
// in here: tests/abi_shims_check.cpp drives the shims with a plain g++ build.
#pragma once

#include <cstdio>
#include <exception>
#include <string>
#include <utility>

#include "engine_interface.h"

namespace pqa {
namespace abi {

inline void AssignErr(void **ppError, Error &err) {  // PqaCInterop.cpp:45-54
  if (!ppError) return;
  *ppError = err.ok() ? nullptr : new Error(std::move(err));
}
inline void *ReturnErr(Error &&err) {  // PqaCInterop.cpp:56-61
  if (err.ok()) return nullptr;
  return new Error(std::move(err));
}
inline Error NullEngine() { return Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of IPqaEngine."); }
inline Error NullFactory() { return Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of IPqaEngineFactory."); }
inline IEngine *AsEngine(void *pvEngine) { return static_cast<pqa::IEngine *>(pvEngine); }

// The barrier: the reference's two exception codes (PqaErrors.h: StdException, SRException).
template <typename Fn>
Error Guarded(Fn &&fn) {
  try {
    return fn();
  } catch (const std::exception &ex) {
    return Error::MakeP(ErrCode::StdException, std::string("what=[") + ex.what() + "]", "A C++ exception was caught at the C interface.");
  } catch (...) {
    return Error::Make(ErrCode::SRException, "An unknown exception was caught at the C interface.");
  }
}
// fn(Error &) -> T behind the barrier: its value and *ppError (a null ppError is tolerated); `fail` with every error.
template <typename T, typename Fn>
T GuardedValue(void **ppError, T fail, Fn &&fn) {
  T v = fail;
  Error err = Guarded([&]() { Error e; v = fn(e); return e; });
  if (!err.ok()) v = fail;
  AssignErr(ppError, err);
  return v;
}

// Returns an error object: fn(IEngine &) -> Error.
template <typename Fn>
void *ErrorOf(void *pvEngine, Fn &&fn) {
  IEngine *pEng = AsEngine(pvEngine);
  if (pEng == nullptr) return new Error(NullEngine());
  return ReturnErr(Guarded([&]() -> Error { return fn(*pEng); }));
}
// Sets *ppError and returns a value: fn(IEngine &, Error &) -> T.
template <typename T, typename Fn>
T ValueOf(void *pvEngine, void **ppError, T fail, Fn &&fn) {
  IEngine *pEng = AsEngine(pvEngine);
  if (pEng == nullptr) {
    if (ppError) *ppError = new Error(NullEngine());
    return fail;
  }
  return GuardedValue<T>(ppError, fail, [&](Error &e) { return fn(*pEng, e); });
}
// Logs and returns a value: fn(IEngine &) -> T.
template <typename T, typename Fn>
T LoggedOf(void *pvEngine, T fail, Fn &&fn) {
  IEngine *pEng = AsEngine(pvEngine);
  if (pEng == nullptr) {
    std::fprintf(stderr, "PqaCore: Nullptr is passed in place of IPqaEngine.\n");
    return fail;
  }
  T v = fail;
  const Error err = Guarded([&]() { v = fn(*pEng); return Error(); });
  if (err.ok()) return v;
  std::fprintf(stderr, "PqaCore: %s %s\n", err.message.c_str(), err.params.c_str());
  return fail;
}
// The factory's entries: fn(Error &) -> IEngine *, a null engine with every error.
template <typename Fn>
void *EngineOf(void *pvFactory, void **ppError, Fn &&fn) {
  if (pvFactory == nullptr) {  // PqaCInterop.cpp:93-98
    if (ppError) *ppError = new Error(NullFactory());
    return nullptr;
  }
  return GuardedValue<IEngine *>(ppError, nullptr, fn);
}

}  // namespace abi
}  // namespace pqa
