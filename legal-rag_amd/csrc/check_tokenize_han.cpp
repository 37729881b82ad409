// Host check of the Han modes of the BM25 query tokeniser (tokenize_rule.hpp through tokenize.cpp's C ABI), a program of
// its own (never part of the library):
//   check_tokenize_han KEYS LOGW WORD LOGW_UNKNOWN TEXTS
//     KEYS, TEXTS   int64 n, int64 offsets[n + 1], then the UTF-8 bytes back to back
//     LOGW          double[n keys];  WORD  uint8[n keys];  LOGW_UNKNOWN  a decimal double
// For AMDR_HAN_CHAR and AMDR_HAN_DICT it cuts every text of TEXTS, and a generated fuzz of byte strings spliced from
// them at ARBITRARY byte positions (so: text that is not UTF-8, characters cut in half, Han lead bytes before ASCII),
// and checks that every span lies inside its text, that the spans tile the text in order without a gap or an empty
// span, and that tokens <= bytes (the span buffers hold exactly `bytes` entries: one more token is an error).  The
// batch entry amdr_tokenizer_encode then has to give the same counts and flag nothing.
// Build: hipcc -x hip --offload-host-only check_tokenize_han.cpp tokenize.cpp (host code only;
// tests/test_han_rule_host.py adds the host sanitizers, which is what makes an access outside the route scratch, the
// dictionary table or the text a failure here).
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "common.hpp"

// the library's plumbing that tokenize.cpp expects from api.cpp
namespace amdr {
std::string& last_error_ref() {
  static thread_local std::string e;
  return e;
}
int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  last_error_ref() = buf;
  return code;
}
std::atomic<long long>& devbuf_growths() {
  static std::atomic<long long> g{0};
  return g;
}
}  // namespace amdr

namespace {

struct Blob {
  std::vector<int64_t> offs;
  std::string bytes;
  int64_t n() const { return (int64_t)offs.size() - 1; }
};

bool read_all(const char* path, std::string* out) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  char buf[65536];
  size_t got;
  while ((got = fread(buf, 1, sizeof buf, f)) > 0) out->append(buf, got);
  fclose(f);
  return true;
}

bool read_blob(const char* path, Blob* b) {
  std::string raw;
  if (!read_all(path, &raw) || raw.size() < 8) return false;
  int64_t n;
  memcpy(&n, raw.data(), 8);
  if (n < 0 || raw.size() < 8 + (size_t)(n + 1) * 8) return false;
  b->offs.resize((size_t)n + 1);
  memcpy(b->offs.data(), raw.data() + 8, (size_t)(n + 1) * 8);
  b->bytes = raw.substr(8 + (size_t)(n + 1) * 8);
  for (int64_t i = 0; i < n; ++i)
    if (b->offs[(size_t)i + 1] < b->offs[(size_t)i]) return false;
  return b->offs[0] == 0 && b->offs[(size_t)n] == (int64_t)b->bytes.size();
}

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return rng_state * 2685821237946237ull;
}

// spans of one text under the handle's mode; returns the token count, or -1 after printing what is wrong
long check_text(const amdr_tokenizer_t* t, const std::string& s, int mode) {
  const int32_t cap = (int32_t)s.size();
  // exactly `bytes` entries, no slack: the sanitizer sees a write behind them
  std::vector<int32_t> st((size_t)cap), en((size_t)cap);
  int32_t n = -2;
  if (amdr_tokenizer_spans_han(t, s.data(), (int64_t)s.size(), st.data(), en.data(), cap, &n) != AMDR_OK) {
    fprintf(stderr, "mode %d: spans_han failed on %zu bytes: %s\n", mode, s.size(), amdr::last_error_ref().c_str());
    return -1;
  }
  if (n < 0 || n > cap) {
    fprintf(stderr, "mode %d: %d tokens for %d bytes\n", mode, n, cap);
    return -1;
  }
  int32_t at = 0;
  for (int32_t i = 0; i < n; ++i) {
    if (st[(size_t)i] != at || en[(size_t)i] <= st[(size_t)i] || en[(size_t)i] > cap) {
      fprintf(stderr, "mode %d: span %d = [%d, %d) does not continue at %d inside %d bytes\n", mode, i, st[(size_t)i],
              en[(size_t)i], at, cap);
      return -1;
    }
    at = en[(size_t)i];
  }
  if (at != cap) {
    fprintf(stderr, "mode %d: the spans end at %d of %d bytes\n", mode, at, cap);
    return -1;
  }
  return n;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 6) {
    fprintf(stderr, "usage: check_tokenize_han KEYS LOGW WORD LOGW_UNKNOWN TEXTS\n");
    return 2;
  }
  Blob keys, texts;
  std::string logw_raw, word_raw;
  if (!read_blob(argv[1], &keys) || !read_all(argv[2], &logw_raw) || !read_all(argv[3], &word_raw) ||
      !read_blob(argv[5], &texts)) {
    fprintf(stderr, "cannot read the inputs\n");
    return 2;
  }
  if (logw_raw.size() != (size_t)keys.n() * 8 || word_raw.size() != (size_t)keys.n()) return 2;
  std::vector<double> logw((size_t)keys.n());
  memcpy(logw.data(), logw_raw.data(), logw_raw.size());
  const double unknown = strtod(argv[4], nullptr);

  // the texts, then splices of their bytes cut anywhere
  std::vector<std::string> all;
  for (int64_t i = 0; i < texts.n(); ++i)
    all.emplace_back(texts.bytes, (size_t)texts.offs[(size_t)i], (size_t)(texts.offs[(size_t)i + 1] - texts.offs[(size_t)i]));
  const size_t given = all.size();
  if (!texts.bytes.empty())
    for (int i = 0; i < 4000; ++i) {
      std::string s;
      const int pieces = 1 + (int)(rnd() % 4);
      for (int p = 0; p < pieces; ++p) {
        const size_t a = (size_t)(rnd() % texts.bytes.size());
        const size_t len = (size_t)(rnd() % 24);
        s.append(texts.bytes, a, len);  // (clamped at the end of the bytes)
        if (rnd() % 8 == 0) s.push_back((char)(rnd() & 0xFF));
      }
      all.push_back(s);
    }

  // a vocabulary of the dictionary's own keys: encode looks tokens up as it does in the library
  long total_tokens = 0;
  for (int mode = AMDR_HAN_CHAR; mode <= AMDR_HAN_DICT; ++mode) {
    amdr_tokenizer_t* t = nullptr;
    if (amdr_tokenizer_create(keys.bytes.data(), keys.offs.data(), keys.n(), &t) != AMDR_OK) return 1;
    if (amdr_tokenizer_set_han(t, mode, keys.bytes.data(), keys.offs.data(), logw.data(),
                               reinterpret_cast<const uint8_t*>(word_raw.data()), keys.n(), unknown) != AMDR_OK) {
      fprintf(stderr, "set_han(%d) failed: %s\n", mode, amdr::last_error_ref().c_str());
      return 1;
    }
    int32_t got_mode = -1;
    if (amdr_tokenizer_han_mode(t, &got_mode) != AMDR_OK || got_mode != mode) return 1;
    std::vector<long> counts;
    for (const std::string& s : all) {
      const long n = check_text(t, s, mode);
      if (n < 0) return 1;
      counts.push_back(n);
      total_tokens += n;
    }
    // the batch entry over the same texts: counts as above, nothing flagged, term ids written for every token
    std::string blob;
    std::vector<int64_t> offs(1, 0);
    for (const std::string& s : all) {
      blob += s;
      offs.push_back((int64_t)blob.size());
    }
    const int32_t nq = (int32_t)all.size();
    std::vector<int32_t> terms(blob.size() ? blob.size() : 1), flags((size_t)nq);
    std::vector<int64_t> q_ptr((size_t)nq + 1);
    if (amdr_tokenizer_encode(t, blob.data(), offs.data(), nq, terms.data(), (int64_t)blob.size(), q_ptr.data(),
                              flags.data()) != AMDR_OK) {
      fprintf(stderr, "mode %d: encode failed: %s\n", mode, amdr::last_error_ref().c_str());
      return 1;
    }
    for (int32_t q = 0; q < nq; ++q)
      if (flags[(size_t)q] != 0 || q_ptr[(size_t)q + 1] - q_ptr[(size_t)q] != counts[(size_t)q]) {
        fprintf(stderr, "mode %d: query %d: flag %d, %lld terms against %ld spans\n", mode, q, flags[(size_t)q],
                (long long)(q_ptr[(size_t)q + 1] - q_ptr[(size_t)q]), counts[(size_t)q]);
        return 1;
      }
    amdr_tokenizer_destroy(t);
  }
  // what set_han refuses
  amdr_tokenizer_t* t = nullptr;
  if (amdr_tokenizer_create(nullptr, nullptr, 0, &t) != AMDR_OK) return 1;
  if (amdr_tokenizer_set_han(t, 3, nullptr, nullptr, nullptr, nullptr, 0, 0.0) != AMDR_EINVAL) return 1;
  if (amdr_tokenizer_set_han(t, AMDR_HAN_DICT, nullptr, nullptr, nullptr, nullptr, 0, unknown) != AMDR_EINVAL) return 1;
  amdr_tokenizer_destroy(t);
  printf("han rule ok: %zu texts (%zu given), %ld tokens\n", all.size(), given, total_tokens);
  return 0;
}
