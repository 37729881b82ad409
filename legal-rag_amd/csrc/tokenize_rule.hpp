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
constexpr uint64_t kFnvInit = 1469598103934665603ull;
constexpr uint64_t kFnvPrime = 1099511628211ull;
AMDR_TOK_HD uint32_t hash_fold(uint64_t h) { return (uint32_t)(h ^ (h >> 32)); }
AMDR_TOK_HD uint32_t hash(const unsigned char* p, long n) {
  uint64_t h = kFnvInit;
  for (long i = 0; i < n; ++i) h = (h ^ p[i]) * kFnvPrime;
  return hash_fold(h);
}

// ---- Han text (include/amdretrieval.h: AMDR_HAN_CHAR, AMDR_HAN_DICT) -----------------------------------------------------
// A sentence that holds a Han character is cut by text.jieba_cut_restated (mode 1: blocks go through finalseg, one Han
// character per token) or by text.dict_cut (mode 2: jieba's default cut over the caller's dictionary, without the HMM).
// A sentence without one takes tokenize() above in every mode.
//
// The dictionary (mode 2) is an open-addressing table over the UTF-8 bytes of its keys — the words and every proper
// prefix of a word — with the vocabulary's hash; per key its log weight (log freq - log total, computed by the caller:
// nothing here takes a logarithm) and the flag "freq > 0".  The hash extends byte by byte, so the prefix walk from one
// position costs one probe per added character.  All pointers are host pointers in tokenize.cpp and device pointers in
// tokenize.hip; the descriptor is passed by value.
struct HanRule {
  int32_t mode = 0;                      // 0: a Han sentence is flagged and gets no tokens
  uint32_t mask = 0;                     // slots - 1 (a power of two)
  int32_t max_key = 0;                   // bytes of the longest key
  const int32_t* slots = nullptr;        // -1 = empty, else a key id
  const int32_t* offs = nullptr;         // key i = blob[offs[i] .. offs[i + 1])
  const unsigned char* blob = nullptr;
  const double* logw = nullptr;          // [keys]
  const unsigned char* is_word = nullptr;  // [keys]: freq > 0
  double logw_unknown = 0.0;             // 0.0 - log total: a key of frequency 0, or no key at all
};

// id of the key p[0 .. n) whose folded hash is h, or -1
AMDR_TOK_HD int32_t han_find(const HanRule& r, const unsigned char* p, int n, uint32_t h) {
  if (n > r.max_key) return -1;
  for (uint32_t i = h & r.mask;; i = (i + 1) & r.mask) {
    const int32_t id = r.slots[i];
    if (id < 0) return -1;
    const int32_t lo = r.offs[id];
    if (r.offs[id + 1] - lo == n) {
      int k = 0;
      while (k < n && r.blob[lo + k] == p[k]) ++k;
      if (k == n) return id;
    }
  }
}

// bytes of the code point at s[i] (i < hi)
AMDR_TOK_HD int cp_len(const unsigned char* s, int i, int hi) {
  int len;
  decode(s + i, s + hi, &len);
  return len;
}

// finalseg on a buffer [lo, hi) of block characters: Han characters one per token, the ASCII runs between them by the
// non-Han rule
template <class Emit>
AMDR_TOK_HD void finalseg_mixed(const unsigned char* s, int lo, int hi, Emit&& emit) {
  int i = lo;
  while (i < hi) {
    if (s[i] < 0x80) {
      int j = i;
      while (j < hi && s[j] < 0x80) ++j;
      finalseg_ascii(s, i, j, emit);
      i = j;
    } else {
      const int len = cp_len(s, i, hi);
      emit(i, i + len);
      i += len;
    }
  }
}

// a buffer of single steps: one character is itself; (mode 2) a buffer that is a word is emitted per character; anything
// else goes through finalseg
template <class Emit>
AMDR_TOK_HD void flush_buffer(const unsigned char* s, int a, int b, const HanRule& han, bool dict, Emit&& emit) {
  if (b <= a) return;
  if (a + cp_len(s, a, b) == b) {
    emit(a, b);
    return;
  }
  if (dict && b - a <= han.max_key) {
    const int32_t id = han_find(han, s + a, b - a, hash(s + a, b - a));
    if (id >= 0 && han.is_word[id]) {
      for (int i = a; i < b;) {
        const int len = cp_len(s, i, b);
        emit(i, i + len);
        i += len;
      }
      return;
    }
  }
  finalseg_mixed(s, a, b, emit);
}

// mode 1: cut_block() for a block that may hold Han characters (text._cut_block)
template <class Emit>
AMDR_TOK_HD void cut_block_char(const unsigned char* s, int lo, int hi, const HanRule& han, Emit&& emit) {
  bool marks = false;
  for (int i = lo; i < hi; ++i) marks |= (s[i] == '&' || s[i] == '+' || s[i] == '#');
  if (!marks) {
    flush_buffer(s, lo, hi, han, false, emit);
    return;
  }
  int buf = lo, i = lo;
  while (i < hi) {
    const int n = dict_word_at(s, i, hi);  // (ASCII bytes only: never inside a multi-byte character)
    if (n) {
      flush_buffer(s, buf, i, han, false, emit);
      emit(i, i + n);
      i += n;
      buf = i;
    } else {
      ++i;
    }
  }
  flush_buffer(s, buf, hi, han, false, emit);
}

// mode 2: text._dict_cut_block.  rv / rx: the route, indexed by the byte offset of a character's first byte (the
// caller's storage, one entry per byte of the sentence); the value behind the block's last character is 0.0 and is not
// stored.  The word graph is not stored either: from the right, each position walks its prefixes forward and keeps
// the best candidate, `>=` so that ties go to the longer word as Python's max() over (value, end) does.
template <class Emit>
AMDR_TOK_HD void cut_block_dict(const unsigned char* s, int lo, int hi, const HanRule& han, double* rv, int32_t* rx,
                                Emit&& emit) {
  // every character's start is linked to the one before it, so that the walk from the right never guesses at a
  // boundary (bytes that are not UTF-8 included: decode() alone says where a character starts)
  int last = -1;
  for (int pos = lo; pos < hi;) {
    rx[pos] = last;
    last = pos;
    pos += cp_len(s, pos, hi);
  }
  for (int idx = last; idx >= lo;) {
    const int before = rx[idx];
    uint64_t h = kFnvInit;
    bool have = false;
    double best = 0.0;
    int best_end = 0, first_end = 0;
    for (int pos = idx; pos < hi;) {
      const int end = pos + cp_len(s, pos, hi);
      for (int k = pos; k < end; ++k) h = (h ^ s[k]) * kFnvPrime;
      if (pos == idx) first_end = end;
      const int32_t id = han_find(han, s + idx, end - idx, hash_fold(h));
      if (id < 0) break;
      if (han.is_word[id]) {
        const double v = han.logw[id] + (end < hi ? rv[end] : 0.0);
        if (!have || v >= best) {
          best = v;
          best_end = end;
          have = true;
        }
      }
      pos = end;
    }
    if (!have) {  // no word starts here: the character alone, at the weight of an unknown word
      best = han.logw_unknown + (first_end < hi ? rv[first_end] : 0.0);
      best_end = first_end;
    }
    rv[idx] = best;
    rx[idx] = best_end;
    idx = before;
  }
  int x = lo, buf = lo;
  while (x < hi) {
    const int one = x + cp_len(s, x, hi);
    int y = rx[x];
    if (y <= x || y > hi) y = one;  // (cannot happen: every start has its route)
    if (y != one) {                 // a word of several characters: the buffer of single steps first
      flush_buffer(s, buf, x, han, true, emit);
      emit(x, y);
      buf = y;
    }
    x = y;
  }
  flush_buffer(s, buf, hi, han, true, emit);
}

// tokens of one sentence under `han`: mode 0, or a sentence without a Han character, is tokenize() above; a Han sentence
// in modes 1 and 2 is cut here and true is returned.  rv / rx: route storage of n entries each (mode 2 only).
template <class Emit>
AMDR_TOK_HD bool tokenize(const unsigned char* s, int n, const HanRule& han, double* rv, int32_t* rx, Emit&& emit) {
  bool is_han_text = false;
  if (han.mode != 0) {
    bool maybe = false;  // U+4E00 .. U+9FD5 start with the bytes E4 .. E9
    for (int i = 0; i < n; ++i) maybe |= (unsigned)(s[i] - 0xE4) <= 5u;
    if (maybe) {
      const unsigned char* end = s + n;
      for (int i = 0; i < n && !is_han_text;) {
        int len;
        is_han_text = is_han(decode(s + i, end, &len));
        i += len;
      }
    }
  }
  if (!is_han_text) return tokenize(s, n, emit);
  const unsigned char* end = s + n;
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
      if (han.mode == 2)
        cut_block_dict(s, i, j, han, rv, rx, emit);
      else
        cut_block_char(s, i, j, han, emit);
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
  // Han text (amdr_tokenizer_set_han): the mode and, for the dictionary mode, the key table `han` points into
  std::string han_blob;
  std::vector<int32_t> han_offs, han_slots;
  std::vector<double> han_logw;
  std::vector<unsigned char> han_word;
  amdr_tok::HanRule han;
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
