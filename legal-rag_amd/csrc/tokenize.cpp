// Query tokeniser + vocabulary lookup of the BM25 channel, native and batched (host code, no device work).
//
// Replaces, per query, `tokens = list(jieba.cut(query))` + the term lookup of rank_bm25's get_scores
// (legalrag/retrieval/bm25_retriever.py:73-74) for text WITHOUT Han characters — the case jieba's default mode
// (cut_all=False, HMM=True) decides without its dictionary; legal-rag_amd/text.py states the rule and is the
// executable specification this file follows token for token (tests/test_text.py compares the two):
//   1. the sentence is split on maximal runs of [一-鿕 a-zA-Z0-9 + # & . _ % -] ("blocks"); between blocks
//      "\r\n" or ONE whitespace character (Python's \s on str: str.isspace()) is a token, every other character is
//      a token of its own;
//   2. a block of one character is that character; a longer block is cut by finalseg's non-Han rule: runs matching
//      [a-zA-Z0-9]+(?:\.\d+)?%? are one token each and each maximal run of the remaining characters is one token;
//      the five ASCII multi-character entries of jieba's dictionary (AT&T, C++, c++, C#, c#) are tokens wherever
//      they start, the text between them is cut as above.
// A query that holds a Han character is, by default, NOT tokenised here (it needs jieba's dictionary): it is flagged and
// the caller takes the Python path (which raises unless a segmenter or an explicit stand-in is configured).  With
// amdr_tokenizer_set_han the handle cuts such a query itself, by one of the two stand-ins of text.py: one Han character
// per token (AMDR_HAN_CHAR, text.jieba_cut_restated) or jieba's default cut over the caller's dictionary without the HMM
// (AMDR_HAN_DICT, text.dict_cut); the flag is then 0 and the terms are written.  tokenize_rule.hpp holds both.
// Queries are NOT lower-cased (the reference does not, bm25_retriever.py:73).  One call handles a whole batch and
// writes the term-id CSR amdr_bm25_search takes; ctypes releases the GIL for its duration.
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <functional>
#include <mutex>
#include <new>
#include <pthread.h>
#include <string>
#include <thread>
#include <vector>

#include "common.hpp"
#include "tokenize_rule.hpp"

namespace {

using amdr_tok::tokenize;

}  // namespace

extern "C" {

int amdr_tokenizer_create(const char* vocab_blob, const int64_t* vocab_offsets, int64_t n_terms,
                          amdr_tokenizer_t** out) {
  AMDR_REQUIRE(out != nullptr, "tokenizer_create: out is null");
  *out = nullptr;
  AMDR_REQUIRE(n_terms >= 0 && n_terms < (1ll << 30) && (n_terms == 0 || (vocab_blob && vocab_offsets)),
               "tokenizer_create: bad vocabulary");
  amdr_tokenizer* t = new (std::nothrow) amdr_tokenizer();
  if (!t) return amdr::fail(AMDR_ENOMEM, "tokenizer_create: host alloc");
  for (int c = 0; c < 256; ++c) t->single[c] = -1;
  for (int64_t i = 0; i < n_terms; ++i) {
    if (vocab_offsets[i + 1] < vocab_offsets[i]) {
      delete t;
      return amdr::fail(AMDR_EINVAL, "tokenizer_create: offsets not ascending at term %lld", (long long)i);
    }
  }
  if (n_terms) {
    const int64_t base = vocab_offsets[0];
    t->blob.assign(vocab_blob + base, (size_t)(vocab_offsets[n_terms] - base));
    t->offs.resize((size_t)n_terms + 1);
    for (int64_t i = 0; i <= n_terms; ++i) t->offs[(size_t)i] = vocab_offsets[i] - base;
    size_t cap = 16;
    while (cap < (size_t)n_terms * 2) cap <<= 1;
    t->slots.assign(cap, -1);
    t->mask = (uint32_t)(cap - 1);
    for (int64_t i = 0; i < n_terms; ++i) {  // first id of a repeated term wins
      const unsigned char* p = reinterpret_cast<const unsigned char*>(t->blob.data()) + t->offs[(size_t)i];
      const size_t n = (size_t)(t->offs[(size_t)i + 1] - t->offs[(size_t)i]);
      if (t->find_slow(p, n) >= 0) continue;
      uint32_t j = amdr_tokenizer::hash(p, n) & t->mask;
      while (t->slots[j] >= 0) j = (j + 1) & t->mask;
      t->slots[j] = (int32_t)i;
      if (n == 1) t->single[p[0]] = (int32_t)i;
    }
  }
  *out = t;
  return AMDR_OK;
}

int amdr_tokenizer_set_han(amdr_tokenizer_t* t, int32_t mode, const char* key_blob, const int64_t* key_offsets,
                           const double* logw, const uint8_t* is_word, int64_t n_keys, double logw_unknown) {
  AMDR_REQUIRE(t != nullptr, "tokenizer_set_han: null handle");
  AMDR_REQUIRE(mode == AMDR_HAN_FLAG || mode == AMDR_HAN_CHAR || mode == AMDR_HAN_DICT, "tokenizer_set_han: bad mode %d",
               mode);
  if (mode != AMDR_HAN_DICT) n_keys = 0;  // the other modes consult no dictionary
  AMDR_REQUIRE(mode != AMDR_HAN_DICT || (n_keys > 0 && n_keys < (1ll << 28) && key_blob && key_offsets && logw && is_word),
               "tokenizer_set_han: the dictionary mode needs keys");
  AMDR_REQUIRE(mode != AMDR_HAN_DICT || std::isfinite(logw_unknown), "tokenizer_set_han: logw_unknown is not finite");
  for (int64_t i = 0; i < n_keys; ++i) {
    AMDR_REQUIRE(key_offsets[i + 1] > key_offsets[i], "tokenizer_set_han: key %lld is empty or its offsets descend",
                 (long long)i);
    AMDR_REQUIRE(std::isfinite(logw[i]), "tokenizer_set_han: logw of key %lld is not finite", (long long)i);
  }
  AMDR_REQUIRE(n_keys == 0 || key_offsets[n_keys] - key_offsets[0] < (1ll << 31), "tokenizer_set_han: keys too long");
  amdr_tok::HanRule han;
  han.mode = mode;
  t->han_blob.clear();
  t->han_offs.clear();
  t->han_slots.clear();
  t->han_logw.clear();
  t->han_word.clear();
  if (n_keys) {
    const int64_t base = key_offsets[0];
    t->han_blob.assign(key_blob + base, (size_t)(key_offsets[n_keys] - base));
    t->han_offs.resize((size_t)n_keys + 1);
    for (int64_t i = 0; i <= n_keys; ++i) t->han_offs[(size_t)i] = (int32_t)(key_offsets[i] - base);
    t->han_logw.assign(logw, logw + n_keys);
    t->han_word.resize((size_t)n_keys);
    for (int64_t i = 0; i < n_keys; ++i) t->han_word[(size_t)i] = is_word[i] ? 1 : 0;
    size_t cap = 16;
    while (cap < (size_t)n_keys * 2) cap <<= 1;
    t->han_slots.assign(cap, -1);
    han.mask = (uint32_t)(cap - 1);
    han.slots = t->han_slots.data();
    han.offs = t->han_offs.data();
    han.blob = reinterpret_cast<const unsigned char*>(t->han_blob.data());
    han.logw = t->han_logw.data();
    han.is_word = t->han_word.data();
    han.logw_unknown = logw_unknown;
    for (int64_t i = 0; i < n_keys; ++i) {
      const int32_t len = t->han_offs[(size_t)i + 1] - t->han_offs[(size_t)i];
      if (len > han.max_key) han.max_key = len;
    }
    for (int64_t i = 0; i < n_keys; ++i) {  // first entry of a repeated key wins
      const unsigned char* p = han.blob + t->han_offs[(size_t)i];
      const int32_t len = t->han_offs[(size_t)i + 1] - t->han_offs[(size_t)i];
      const uint32_t h = amdr_tok::hash(p, len);
      if (amdr_tok::han_find(han, p, len, h) >= 0) continue;
      uint32_t j = h & han.mask;
      while (t->han_slots[j] >= 0) j = (j + 1) & han.mask;
      t->han_slots[j] = (int32_t)i;
    }
  }
  t->han = han;
  return AMDR_OK;
}

int amdr_tokenizer_han_mode(const amdr_tokenizer_t* t, int32_t* mode) {
  AMDR_REQUIRE(t != nullptr && mode != nullptr, "tokenizer_han_mode: null argument");
  *mode = t->han.mode;
  return AMDR_OK;
}

}  // extern "C"

namespace {

// A small persistent pool: a batch of tens of thousands of queries is cut into ranges, one per worker; starting
// std::threads per call cost more than tokenising a few thousand queries.  Workers sleep on a condition variable
// between calls; calls from several Python threads are serialised on the pool (each still runs on all workers).
class Pool {
 public:
  static Pool& get() {
    // never destroyed: no join at process exit (detached daemon threads).  A forked child has none of the parent's
    // threads: it starts its own pool at its first batch.
    static std::once_flag once;
    std::call_once(once, [] { pthread_atfork(nullptr, nullptr, [] { inst().store(nullptr); }); });
    Pool* p = inst().load();
    if (!p) {
      static std::mutex mk;
      std::lock_guard<std::mutex> g(mk);
      p = inst().load();
      if (!p) {
        p = new Pool();
        inst().store(p);
      }
    }
    return *p;
  }
  static std::atomic<Pool*>& inst() {
    static std::atomic<Pool*> i{nullptr};
    return i;
  }
  int workers() const { return (int)th_.size() + 1; }
  // fn(part) for part = 0 .. parts - 1, parts <= workers(); the caller runs part 0
  void run(int parts, const std::function<void(int)>& fn) {
    if (parts <= 1) {
      fn(0);
      return;
    }
    std::lock_guard<std::mutex> call(call_mu_);
    {
      std::lock_guard<std::mutex> g(mu_);
      fn_ = &fn;
      parts_ = parts;
      pending_ = parts - 1;
      ++gen_;
    }
    cv_.notify_all();
    fn(0);
    std::unique_lock<std::mutex> g(mu_);
    done_.wait(g, [&] { return pending_ == 0; });
    fn_ = nullptr;
  }

 private:
  Pool() {
    int n = (int)std::thread::hardware_concurrency();
    const char* e = getenv("AMDR_TOKENIZER_THREADS");
    if (e && atoi(e) >= 1) n = atoi(e);
    if (n > 32) n = 32;
    if (n < 1) n = 1;
    for (int i = 1; i < n; ++i) {
      th_.emplace_back([this, i] { loop(i); });
      th_.back().detach();
    }
  }
  void loop(int id) {
    uint64_t seen = 0;
    for (;;) {
      const std::function<void(int)>* fn = nullptr;
      {
        std::unique_lock<std::mutex> g(mu_);
        cv_.wait(g, [&] { return gen_ != seen; });
        seen = gen_;
        if (id < parts_) fn = fn_;
      }
      if (fn) {
        (*fn)(id);
        std::lock_guard<std::mutex> g(mu_);
        if (--pending_ == 0) done_.notify_one();
      }
    }
  }
  std::vector<std::thread> th_;
  std::mutex mu_, call_mu_;
  std::condition_variable cv_, done_;
  const std::function<void(int)>* fn_ = nullptr;
  int parts_ = 0, pending_ = 0;
  uint64_t gen_ = 0;
};

// the batch core: query q = the lens[q] bytes at ptrs[q] -> CSR.  Two phases: every worker tokenises its range of
// queries into its own term buffer (+ per-query counts), then the prefix sum over the counts gives q_ptr and every
// worker copies its terms to their place.
int encode_core(const amdr_tokenizer* t, const unsigned char* const* ptrs, const int64_t* lens, int32_t nq,
                int32_t* term_ids, int64_t capacity, int64_t* q_ptr, int32_t* needs_segmenter) {
  if (nq == 0) return AMDR_OK;
  q_ptr[0] = 0;
  Pool& pool = Pool::get();
  int parts = pool.workers();
  if (parts > nq / 256) parts = nq / 256;  // a worker is worth waking for a few hundred queries
  if (parts < 1) parts = 1;
  std::vector<std::vector<int32_t>> bufs((size_t)parts);
  std::atomic<int> bad{-1};
  auto range = [&](int p, int32_t* lo, int32_t* hi) {
    *lo = (int32_t)((int64_t)nq * p / parts);
    *hi = (int32_t)((int64_t)nq * (p + 1) / parts);
  };
  std::function<void(int)> phase1 = [&](int p) {
    int32_t lo, hi;
    range(p, &lo, &hi);
    std::vector<int32_t>& out = bufs[(size_t)p];
    int64_t bytes = 0;
    for (int32_t q = lo; q < hi; ++q) bytes += lens[q] > 0 ? lens[q] : 0;
    out.reserve((size_t)(bytes / 2 + 16));
    const amdr_tok::HanRule han = t->han;
    std::vector<double> rv;  // this worker's route scratch (dictionary mode), grown to its longest query
    std::vector<int32_t> rx;
    for (int32_t q = lo; q < hi; ++q) {
      const int64_t n = lens[q];
      if (n < 0 || n >= (1ll << 31) || (n > 0 && !ptrs[q])) {
        bad.store(q);
        return;
      }
      const unsigned char* s = ptrs[q];
      const size_t start = out.size();
      if (han.mode == AMDR_HAN_DICT && (size_t)n > rv.size()) {
        rv.resize((size_t)n);
        rx.resize((size_t)n);
      }
      const bool ok = tokenize(s, (int)n, han, rv.data(), rx.data(),
                               [&](int x, int y) { out.push_back(t->find(s + x, (size_t)(y - x))); });
      if (!ok) out.resize(start);
      needs_segmenter[q] = ok ? 0 : 1;
      q_ptr[q + 1] = (int64_t)(out.size() - start);  // the count; turned into the offset below
    }
  };
  pool.run(parts, phase1);
  AMDR_REQUIRE(bad.load() < 0, "tokenizer_encode: bad text at query %d", bad.load());
  for (int32_t q = 0; q < nq; ++q) q_ptr[q + 1] += q_ptr[q];
  AMDR_REQUIRE(q_ptr[nq] <= capacity, "tokenizer_encode: term buffer too small (capacity %lld, %lld terms)",
               (long long)capacity, (long long)q_ptr[nq]);
  std::function<void(int)> phase2 = [&](int p) {
    int32_t lo, hi;
    range(p, &lo, &hi);
    const std::vector<int32_t>& src = bufs[(size_t)p];
    if (!src.empty()) memcpy(term_ids + q_ptr[lo], src.data(), src.size() * sizeof(int32_t));
  };
  pool.run(parts, phase2);
  return AMDR_OK;
}

// offsets into one blob -> pointer / length arrays (`trim` bytes of separator behind every query but the last)
int encode_offsets(const amdr_tokenizer* t, const unsigned char* text, const int64_t* offs, int64_t trim, int32_t nq,
                   int32_t* term_ids, int64_t capacity, int64_t* q_ptr, int32_t* needs_segmenter) {
  std::vector<const unsigned char*> ptrs((size_t)nq);
  std::vector<int64_t> lens((size_t)nq);
  for (int32_t q = 0; q < nq; ++q) {
    ptrs[(size_t)q] = text + offs[q];
    lens[(size_t)q] = offs[q + 1] - offs[q] - (q + 1 < nq ? trim : 0);
  }
  return encode_core(t, ptrs.data(), lens.data(), nq, term_ids, capacity, q_ptr, needs_segmenter);
}

}  // namespace

extern "C" {

int amdr_tokenizer_encode(const amdr_tokenizer_t* t, const char* text_blob, const int64_t* text_offsets, int32_t nq,
                          int32_t* term_ids, int64_t capacity, int64_t* q_ptr, int32_t* needs_segmenter) {
  AMDR_REQUIRE(t != nullptr, "tokenizer_encode: null handle");
  AMDR_REQUIRE(nq >= 0 && (nq == 0 || (text_offsets && q_ptr && needs_segmenter)), "tokenizer_encode: null buffer");
  AMDR_REQUIRE(capacity >= 0 && (capacity == 0 || term_ids), "tokenizer_encode: null term buffer");
  return encode_offsets(t, reinterpret_cast<const unsigned char*>(text_blob), text_offsets, 0, nq, term_ids, capacity, q_ptr,
                        needs_segmenter);
}

int amdr_tokenizer_encode_ptrs(const amdr_tokenizer_t* t, const char* const* texts, const int64_t* n_bytes, int32_t nq,
                               int32_t* term_ids, int64_t capacity, int64_t* q_ptr, int32_t* needs_segmenter) {
  AMDR_REQUIRE(t != nullptr, "tokenizer_encode_ptrs: null handle");
  AMDR_REQUIRE(nq >= 0 && (nq == 0 || (texts && n_bytes && q_ptr && needs_segmenter)), "tokenizer_encode_ptrs: null buffer");
  AMDR_REQUIRE(capacity >= 0 && (capacity == 0 || term_ids), "tokenizer_encode_ptrs: null term buffer");
  return encode_core(t, reinterpret_cast<const unsigned char* const*>(texts), n_bytes, nq, term_ids, capacity, q_ptr,
                     needs_segmenter);
}

int amdr_tokenizer_encode_joined(const amdr_tokenizer_t* t, const char* text_blob, int64_t n_bytes, int32_t nq,
                                 int32_t* term_ids, int64_t capacity, int64_t* q_ptr, int32_t* needs_segmenter) {
  AMDR_REQUIRE(t != nullptr, "tokenizer_encode_joined: null handle");
  AMDR_REQUIRE(nq >= 0 && n_bytes >= 0 && (nq == 0 || (q_ptr && needs_segmenter)), "tokenizer_encode_joined: null buffer");
  AMDR_REQUIRE(n_bytes == 0 || text_blob, "tokenizer_encode_joined: null text");
  AMDR_REQUIRE(capacity >= 0 && (capacity == 0 || term_ids), "tokenizer_encode_joined: null term buffer");
  if (nq == 0) return AMDR_OK;
  // queries are separated by ONE NUL byte (nq - 1 of them): offsets from a memchr walk
  std::vector<int64_t> offs((size_t)nq + 1);
  offs[0] = 0;
  const char* p = text_blob;
  const char* end = text_blob + n_bytes;
  for (int32_t q = 1; q < nq; ++q) {
    const char* z = p < end ? static_cast<const char*>(memchr(p, 0, (size_t)(end - p))) : nullptr;
    AMDR_REQUIRE(z != nullptr, "tokenizer_encode_joined: %d queries announced, separator %d missing", nq, q);
    offs[(size_t)q] = (z - text_blob) + 1;
    p = z + 1;
  }
  AMDR_REQUIRE(p > end || memchr(p, 0, (size_t)(end - p)) == nullptr, "tokenizer_encode_joined: more separators than queries");
  offs[(size_t)nq] = n_bytes;
  return encode_offsets(t, reinterpret_cast<const unsigned char*>(text_blob), offs.data(), 1, nq, term_ids, capacity, q_ptr,
                        needs_segmenter);
}

int amdr_tokenizer_pack(const char* const* texts, const int64_t* n_bytes, int32_t nq, char* blob, int64_t capacity,
                        int64_t* offsets) {
  AMDR_REQUIRE(nq >= 0 && offsets && (nq == 0 || (texts && n_bytes)), "tokenizer_pack: null buffer");
  AMDR_REQUIRE(capacity >= 0 && (capacity == 0 || blob), "tokenizer_pack: null blob");
  int64_t tot = 0;
  for (int32_t q = 0; q < nq; ++q) {
    AMDR_REQUIRE(n_bytes[q] >= 0 && (n_bytes[q] == 0 || texts[q]), "tokenizer_pack: bad text at query %d", q);
    tot += n_bytes[q];
  }
  AMDR_REQUIRE(tot <= capacity, "tokenizer_pack: blob too small (capacity %lld, %lld bytes)", (long long)capacity,
               (long long)tot);
  offsets[0] = 0;
  for (int32_t q = 0; q < nq; ++q) offsets[q + 1] = offsets[q] + n_bytes[q];
  // the copies on the tokeniser's worker pool: one range of queries per worker, as encode_core cuts them
  Pool& pool = Pool::get();
  int parts = pool.workers();
  if (parts > nq / 1024) parts = nq / 1024;
  if (parts < 1) parts = 1;
  std::function<void(int)> copy = [&](int p) {
    const int32_t lo = (int32_t)((int64_t)nq * p / parts), hi = (int32_t)((int64_t)nq * (p + 1) / parts);
    for (int32_t q = lo; q < hi; ++q)
      if (n_bytes[q]) memcpy(blob + offsets[q], texts[q], (size_t)n_bytes[q]);
  };
  pool.run(parts, copy);
  return AMDR_OK;
}

int amdr_tokenizer_spans(const char* text, int64_t n_bytes, int32_t* starts, int32_t* ends, int32_t capacity,
                         int32_t* n_tokens) {
  AMDR_REQUIRE(n_tokens != nullptr && n_bytes >= 0 && n_bytes < (1ll << 31), "tokenizer_spans: bad arguments");
  AMDR_REQUIRE(n_bytes == 0 || text, "tokenizer_spans: null text");
  AMDR_REQUIRE(capacity >= 0 && (capacity == 0 || (starts && ends)), "tokenizer_spans: null span buffers");
  int32_t n = 0;
  bool overflow = false;
  const bool ok = tokenize(reinterpret_cast<const unsigned char*>(text), (int)n_bytes, [&](int a, int b) {
    if (n >= capacity) {
      overflow = true;
      return;
    }
    starts[n] = a;
    ends[n] = b;
    ++n;
  });
  AMDR_REQUIRE(!overflow, "tokenizer_spans: span buffers too small");
  *n_tokens = ok ? n : -1;  // -1: the text holds a Han character and needs a segmenter
  return AMDR_OK;
}

int amdr_tokenizer_spans_han(const amdr_tokenizer_t* t, const char* text, int64_t n_bytes, int32_t* starts, int32_t* ends,
                             int32_t capacity, int32_t* n_tokens) {
  AMDR_REQUIRE(t != nullptr, "tokenizer_spans_han: null handle");
  AMDR_REQUIRE(n_tokens != nullptr && n_bytes >= 0 && n_bytes < (1ll << 31), "tokenizer_spans_han: bad arguments");
  AMDR_REQUIRE(n_bytes == 0 || text, "tokenizer_spans_han: null text");
  AMDR_REQUIRE(capacity >= 0 && (capacity == 0 || (starts && ends)), "tokenizer_spans_han: null span buffers");
  std::vector<double> rv;
  std::vector<int32_t> rx;
  if (t->han.mode == AMDR_HAN_DICT) {
    rv.resize((size_t)n_bytes);
    rx.resize((size_t)n_bytes);
  }
  int32_t n = 0;
  bool overflow = false;
  const bool ok = tokenize(reinterpret_cast<const unsigned char*>(text), (int)n_bytes, t->han, rv.data(), rx.data(),
                           [&](int a, int b) {
                             if (n >= capacity) {
                               overflow = true;
                               return;
                             }
                             starts[n] = a;
                             ends[n] = b;
                             ++n;
                           });
  AMDR_REQUIRE(!overflow, "tokenizer_spans_han: span buffers too small");
  *n_tokens = ok ? n : -1;  // -1: Han text under AMDR_HAN_FLAG
  return AMDR_OK;
}

int amdr_tokenizer_destroy(amdr_tokenizer_t* t) {
  delete t;
  return AMDR_OK;
}

}  // extern "C"
