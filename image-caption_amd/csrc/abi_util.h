// capgen — what every C-ABI function (api.hip, hooks.hip) is made of: the error guard and its
// thread-local message, the dtype and handle checks, the stream hand-off of a decode call, the
// string hand-back and the range check of a capgen_decode_constraints.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <exception>
#include <string>

#include "../../include/capgen.h"
#include "capgen_common.h"
#include "select.h"

namespace capgen {

// capgen_last_error's message: ONE definition, in api.hip (a second one would link, and lose every
// message raised in the other file)
extern thread_local std::string g_last_error;

template <class F>
int guarded(F&& f) {
  try {
    f();
    return 0;
  } catch (const Error& e) {
    g_last_error = e.msg;
  } catch (const std::exception& e) {
    g_last_error = e.what();
  } catch (...) {
    g_last_error = "unknown error";
  }
  return 1;
}

inline DType dt(int x) {
  require(x == CAPGEN_F32 || x == CAPGEN_BF16, "dtype must be CAPGEN_F32 or CAPGEN_BF16");
  return x == CAPGEN_F32 ? DType::F32 : DType::BF16;
}

// (templates over the handle type: this header does not need the engine's definition, which the
// handle-free hooks never read)
template <class H>
void set_device(H* h) {
  require(h != nullptr, "null engine handle");
  CAPGEN_HIP(hipSetDevice(h->device));
}

// a decode entry point: body() enqueued on the engine's stream between the caller's stream's events
// (an exception leaves the engine's stream unjoined, as it may have left it half-enqueued)
template <class H, class F>
int decode_call(H* h, void* stream, F&& body) {
  return guarded([&] {
    set_device(h);
    hipStream_t cs = (hipStream_t)stream;
    h->enter(cs);
    body();
    h->leave(cs);
  });
}

// s into the caller's buffer of cap bytes, cut to fit and 0-terminated (nothing without a buffer)
inline void copy_out(const std::string& s, char* out, int cap) {
  if (!out || cap <= 0) return;
  const size_t k = std::min<size_t>(s.size(), (size_t)cap - 1);
  std::memcpy(out, s.data(), k);
  out[k] = 0;
}

// The ranges of a capgen_decode_constraints for a vocabulary of V words and captions of T = max_length
// (0: not known, the kernel hook) -> the launcher's form, its banned list still the caller's host array.
inline DecodeConstraints checked_constraints(const capgen_decode_constraints& c, int V, int T, const std::string& who) {
  require(c.no_repeat_ngram >= 0 && (T == 0 || c.no_repeat_ngram < T),
          who + ": no_repeat_ngram must be 0 or in [1, max_length)");
  require(c.end_id >= -1 && c.end_id < V, who + ": end_id must be in [-1, num_vocab)");
  require(c.min_length >= 0 && (T == 0 || c.min_length <= T - 1), who + ": min_length must be 0 or in [1, max_length - 1]");
  require(c.min_length == 0 || c.end_id >= 0, who + ": min_length needs an end_id >= 0");
  require(c.repetition_penalty > 0.f && c.repetition_penalty < INFINITY,
          who + ": repetition_penalty must be finite and > 0");  // (false for a NaN)
  require(c.n_banned >= 0 && c.n_banned <= 1024, who + ": n_banned must be in [0, 1024]");
  require(c.n_banned == 0 || c.banned != nullptr, who + ": null banned list with n_banned > 0");
  for (int i = 0; i < c.n_banned; ++i)
    require(c.banned[i] >= 0 && c.banned[i] < V,
            who + ": banned[" + std::to_string(i) + "] = " + std::to_string(c.banned[i]) + " must be in [0, num_vocab)");
  DecodeConstraints d;
  d.no_repeat_ngram = c.no_repeat_ngram, d.min_length = c.min_length, d.end_id = c.end_id;
  d.repetition_penalty = c.repetition_penalty, d.banned = c.banned, d.n_banned = c.n_banned;
  return d;
}

}  // namespace capgen
