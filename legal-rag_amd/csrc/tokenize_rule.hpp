// The BM25 query tokeniser's rule and vocabulary hash, ONE source for the host (tokenize.cpp) and the device
// (tokenize.hip): every function here is __host__ __device__, so the two cannot drift.  legal-rag_amd/text.py is the
// executable specification; the rule is stated in tokenize.cpp's header comment.
//
// `emit(lo, hi)` receives each token's byte range [lo, hi) relative to the sentence start, in order.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace amdr_tok {

// always inlined: a device kernel that calls tokenize() on an LDS copy and on global memory then keeps each call's
// address space (an out-of-line call would take a flat pointer and its lambda through scratch)
#define AMDR_TOK_HD __host__ __device__ inline __attribute__((always_inline))

AMDR_TOK_HD bool is_alnum(uint32_t c) { return (c >= '0' && c <= '9') || (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z'); }
AMDR_TOK_HD bool is_digit(uint32_t c) { return c >= '0' && c <= '9'; }
AMDR_TOK_HD bool is_han(uint32_t c) { return c >= 0x4E00 && c <= 0x9FD5; }
AMDR_TOK_HD bool is_block(uint32_t c) {
  return is_alnum(c) || is_han(c) || c == '+' || c == '#' || c == '&' || c == '.' || c == '_' || c == '%' || c == '-';
}
// Python str.isspace() == what \s matches in a str pattern
AMDR_TOK_HD bool is_space(uint32_t c) {
  return (c >= 0x09 && c <= 0x0D) || (c >= 0x1C && c <= 0x20) || c == 0x85 || c == 0xA0 || c == 0x1680 ||
         (c >= 0x2000 && c <= 0x200A) || c == 0x2028 || c == 0x2029 || c == 0x202F || c == 0x205F || c == 0x3000;
}

// block class of one byte of pure-ASCII text ([a-zA-Z0-9+#&._%-]) as two 64-bit masks: no table in memory, the same
// code on both sides
AMDR_TOK_HD bool ascii_block(unsigned char c) {
  // bits 0-63: '#'(35) '%'(37) '&'(38) '+'(43) '-'(45) '.'(46) '0'-'9'(48-57)
  constexpr uint64_t kLo = (1ull << 35) | (1ull << 37) | (1ull << 38) | (1ull << 43) | (1ull << 45) | (1ull << 46) |
                           (0x3FFull << 48);
  // bits 64-127: 'A'-'Z'(65-90) '_'(95) 'a'-'z'(97-122)
  constexpr uint64_t kHi = (0x3FFFFFFull << 1) | (1ull << 31) | (0x3FFFFFFull << 33);
  return c < 64 ? ((kLo >> c) & 1) != 0 : c < 128 ? ((kHi >> (c - 64)) & 1) != 0 : false;
}

// decode one UTF-8 code point at p (< end); malformed bytes are taken one at a time (Python str input cannot be
// malformed; this only keeps the scan inside the buffer)
AMDR_TOK_HD uint32_t decode(const unsigned char* p, const unsigned char* end, int* len) {
  const unsigned char b = *p;
  if (b < 0x80) {
    *len = 1;
    return b;
  }
  int n = (b >= 0xF0) ? 4 : (b >= 0xE0) ? 3 : (b >= 0xC0) ? 2 : 1;
  if (n == 1 || p + n > end) {
    *len = 1;
    return 0xFFFD;
  }
  uint32_t c = b & (0xFF >> (n + 1));
  for (int i = 1; i < n; ++i) c = (c << 6) | (p[i] & 0x3F);
  *len = n;
  return c;
}

// finalseg's non-Han rule on an ASCII buffer [lo, hi)
template <class Emit>
AMDR_TOK_HD void finalseg_ascii(const unsigned char* s, int lo, int hi, Emit&& emit) {
  int i = lo;
  while (i < hi) {
    int j = i;
    if (is_alnum(s[i])) {
      while (j < hi && is_alnum(s[j])) ++j;
      if (j + 1 < hi && s[j] == '.' && is_digit(s[j + 1])) {
        ++j;
        while (j < hi && is_digit(s[j])) ++j;
      }
      if (j < hi && s[j] == '%') ++j;
    } else {
      while (j < hi && !is_alnum(s[j])) ++j;
    }
    emit(i, j);
    i = j;
  }
}

// length of an ASCII dictionary word (AT&T, C++, c++, C#, c#: the order of jieba's lookup) starting at i, or 0
AMDR_TOK_HD int dict_word_at(const unsigned char* s, int i, int hi) {
  const int n = hi - i;
  if (n >= 4 && s[i] == 'A' && s[i + 1] == 'T' && s[i + 2] == '&' && s[i + 3] == 'T') return 4;
  if (n >= 3 && (s[i] == 'C' || s[i] == 'c') && s[i + 1] == '+' && s[i + 2] == '+') return 3;
  if (n >= 2 && (s[i] == 'C' || s[i] == 'c') && s[i + 1] == '#') return 2;
  return 0;
}

// a block without Han characters (ASCII by construction)
template <class Emit>
AMDR_TOK_HD void cut_block(const unsigned char* s, int lo, int hi, Emit&& emit) {
  bool marks = false;
  for (int i = lo; i < hi; ++i) marks |= (s[i] == '&' || s[i] == '+' || s[i] == '#');
  auto flush = [&](int a, int b) {
    if (b - a == 1)
      emit(a, b);
    else if (b > a)
      finalseg_ascii(s, a, b, emit);
  };
  if (!marks) {
    flush(lo, hi);
    return;
  }
  int buf = lo, i = lo;
  while (i < hi) {
    const int n = dict_word_at(s, i, hi);
    if (n) {
      flush(buf, i);
      emit(i, i + n);
      i += n;
      buf = i;
    } else {
      ++i;
    }
  }
  flush(buf, hi);
}

// tokens of one sentence; returns false (nothing is emitted) when it holds a Han character
template <class Emit>
AMDR_TOK_HD bool tokenize(const unsigned char* s, int n, Emit&& emit) {
  // pure ASCII (every English query): no decoding, no Han check, one mask test per byte — the same rule
  bool ascii = true;
  for (int i = 0; i < n; ++i) ascii &= s[i] < 0x80;
  if (ascii) {
    int i = 0;
    while (i < n) {
      if (ascii_block(s[i])) {
        int j = i + 1;
        while (j < n && ascii_block(s[j])) ++j;
        cut_block(s, i, j, emit);
        i = j;
      } else if (s[i] == '\r' && i + 1 < n && s[i + 1] == '\n') {
        emit(i, i + 2);
        i += 2;
      } else {
        emit(i, i + 1);
        ++i;
      }
    }
    return true;
  }
  const unsigned char* end = s + n;
  for (int i = 0; i < n;) {  // Han anywhere -> the whole sentence goes to the caller's segmenter
    int len;
    if (is_han(decode(s + i, end, &len))) return false;
    i += len;
  }
  int i = 0;
  while (i < n) {
    int len;
    const uint32_t c = decode(s + i, end, &len);
    if (is_block(c)) {
      int j = i;
      while (j < n) {
        int l2;
        if (!is_block(decode(s + j, end, &l2))) break;
        j += l2;
      }
      cut_block(s, i, j, emit);
      i = j;
    } else if (c == '\r' && i + 1 < n && s[i + 1] == '\n') {
      emit(i, i + 2);
      i += 2;
    } else {  // one whitespace character, or any other character on its own
      emit(i, i + len);
      i += len;
    }
  }
  return true;
}

// the vocabulary's hash: FNV-1a, folded to 32 bits (the open-addressing table of amdr_tokenizer and its device copy)
AMDR_TOK_HD uint32_t hash(const unsigned char* p, long n) {
  uint64_t h = 1469598103934665603ull;
  for (long i = 0; i < n; ++i) h = (h ^ p[i]) * 1099511628211ull;
  return (uint32_t)(h ^ (h >> 32));
}

#undef AMDR_TOK_HD

}  // namespace amdr_tok

// The host vocabulary (amdr_tokenizer_t) as an open-addressing table over ONE copy of the term bytes: a lookup hashes
// the token's bytes where they lie in the query (no std::string is built per token) and compares with memcmp.  The
// device copy (tokenize.hip) takes these arrays as they are, so hash, probe order and "first id of a repeated term
// wins" are the host's by construction.
struct amdr_tokenizer {
  std::string blob;               // all terms, back to back
  std::vector<int64_t> offs;      // term i = blob[offs[i] .. offs[i + 1])
  std::vector<int32_t> slots;     // -1 = empty, else a term id; size = power of two >= 2 x terms
  uint32_t mask = 0;
  int32_t single[256];            // one-byte tokens (blanks and punctuation are two thirds of a query's tokens): direct
  static inline uint32_t hash(const unsigned char* p, size_t n) { return amdr_tok::hash(p, (long)n); }
  inline int32_t find(const unsigned char* p, size_t n) const {
    if (n == 1) return single[p[0]];
    return find_slow(p, n);
  }
  inline int32_t find_slow(const unsigned char* p, size_t n) const {
    if (slots.empty()) return -1;
    for (uint32_t i = hash(p, n) & mask;; i = (i + 1) & mask) {
      const int32_t id = slots[i];
      if (id < 0) return -1;
      const int64_t lo = offs[id];
      if ((size_t)(offs[id + 1] - lo) == n && memcmp(blob.data() + lo, p, n) == 0) return id;
    }
  }
};
