// Host check of the rules of amdr_bm25_marks (marks_rule.hpp, over near_rule.hpp's run length), a program of its own:
//   check_marks
// It walks generated documents as the kernel of marks.hip does — round by round and lane by lane: the masks of a round
// staged in an array of exactly mk_run_len words (79 at most), the cover in one of exactly kMkStage words with its tail
// carried into the next round, the marks compacted in lane order into lists of exactly kMkMaxMarks entries, the window
// search 64 anchors per round with the arg-max by mk_better — and compares window, score bits, masks, marks, counts and
// status with a naive scan of whole documents.  Every array has exactly the size the header promises, so with the host
// sanitizers (tests/test_marks_rule_host.py) an access outside one is a failure.  Then written-out cases and every refusal
// of mk_validate.
// Build: c++ -std=c++17 check_marks.cpp (plain host code; no HIP header is needed).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "marks_rule.hpp"

using namespace amdr;

namespace {

int failures = 0;
#define CHECK(cond, ...)                 \
  do {                                   \
    if (!(cond)) {                       \
      ++failures;                        \
      std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      std::printf(__VA_ARGS__);          \
      std::printf("\n");                 \
    }                                    \
  } while (0)

struct Rng {
  uint64_t s;
  uint32_t next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(s >> 33);
  }
  long below(long n) { return (long)(next() % (uint32_t)n); }
};

struct Query {
  std::vector<int> terms, slot;  // the mark table, at exactly its size
  std::vector<double> w;         // 32
  unsigned loose;
  std::vector<std::vector<int>> seqs;
};

struct Result {
  int win[4];
  double score;
  unsigned slots[2];
  std::vector<int> marks;  // [cap, 2]
  int status;
};

bool same(const Result& a, const Result& b) {
  return std::memcmp(a.win, b.win, sizeof a.win) == 0 && std::memcmp(&a.score, &b.score, 8) == 0 &&
         a.slots[0] == b.slots[0] && a.slots[1] == b.slots[1] && a.marks == b.marks && a.status == b.status;
}

// the naive scan: whole documents, no rounds, a linear search in the table
Result naive(const std::vector<int>& doc, const Query& q, int W, int cap) {
  const long n = (long)doc.size();
  std::vector<unsigned> mask((size_t)n, 0u), cover((size_t)n, 0u);
  for (long p = 0; p < n; ++p)
    for (size_t i = 0; i < q.terms.size(); ++i)
      if (q.terms[i] == doc[(size_t)p] && q.slot[i] >= 0 && q.slot[i] < 32) mask[(size_t)p] = 1u << q.slot[i];
  for (const auto& sq : q.seqs) {
    const long L = (long)sq.size();
    if (L < 2 || L > 16 || std::any_of(sq.begin(), sq.end(), [](int s) { return s < 0 || s > 31; })) continue;
    for (long p = 0; p + L <= n; ++p) {
      bool all = true;
      for (long j = 0; j < L && all; ++j) all = (mask[(size_t)(p + j)] >> sq[(size_t)j]) & 1u;
      for (long j = 0; j < L && all; ++j) cover[(size_t)(p + j)] |= 1u << sq[(size_t)j];
    }
  }
  std::vector<std::pair<int, int>> every;
  for (long p = 0; p < n; ++p) {
    const unsigned m = (mask[(size_t)p] & q.loose) | cover[(size_t)p];
    if (m) every.push_back({(int)p, __builtin_ctz(m)});
  }
  std::vector<std::pair<int, int>> kept(every.begin(), every.begin() + std::min<size_t>(every.size(), kMkMaxMarks));
  Result r{};
  r.marks.assign((size_t)cap * 2, -1);
  r.win[0] = 0, r.win[1] = (int)std::min<long>(W, n), r.win[2] = 0, r.win[3] = (int)every.size();
  r.score = 0.0, r.status = every.size() > (size_t)kMkMaxMarks;
  for (auto& m : kept) r.slots[1] |= 1u << m.second;
  bool have = false;
  for (size_t i = 0; i < kept.size(); ++i) {
    const long e = std::min<long>((long)kept[i].first + W, n);
    unsigned bits = 0;
    size_t t = i;
    for (; t < kept.size() && kept[t].first < e; ++t) bits |= 1u << kept[t].second;
    double sc = 0.0;
    for (int s = 0; s < 32; ++s)
      if ((bits >> s) & 1u) sc += q.w[(size_t)s];
    if (!have || sc > r.score) {
      have = true, r.score = sc, r.slots[0] = bits;
      r.win[0] = kept[i].first, r.win[1] = (int)e, r.win[2] = (int)(t - i);
      r.marks.assign((size_t)cap * 2, -1);
      for (size_t j = 0; j < (size_t)cap && j < t - i; ++j) r.marks[2 * j] = kept[i + j].first, r.marks[2 * j + 1] = kept[i + j].second;
    }
  }
  return r;
}

long long longest_run = 0, most_marks = 0;

// one pair as one wave of marks.hip walks it; `stream` holds the document at [begin, end) among its neighbours
Result wave(const std::vector<int>& stream, long long begin, long long end, const Query& q, int W, int cap) {
  const MkTable T{q.terms.data(), q.slot.data(), (long long)q.terms.size()};
  std::vector<int> m_pos((size_t)kMkMaxMarks, -7);
  std::vector<unsigned char> m_slot((size_t)kMkMaxMarks, 0xEE);
  std::vector<unsigned> cover((size_t)kMkStage, 0u);
  const long long doc_len = end - begin;
  int n_marks = 0;
  unsigned kept_slots = 0;
  for (long long base = begin; base < end; base += kPhLanes) {
    const int len = mk_run_len(base, end);
    CHECK(len >= 1 && len <= kMkStage && base + len <= end, "a run of %d masks", len);
    longest_run = std::max<long long>(longest_run, len);
    std::vector<unsigned> run((size_t)len);  // the staged masks, at exactly their size
    for (int lane = 0; lane < kPhLanes; ++lane)
      for (int j = lane; j < len; j += kPhLanes) run[(size_t)j] = mk_token_mask(stream[(size_t)(base + j)], T);
    for (const auto& sq : q.seqs) {
      const long long L = (long long)sq.size();
      if (L < 2 || L > kPhMaxLen || !mk_seq_sized(sq.data(), L)) continue;
      for (int lane = 0; lane < kPhLanes; ++lane)
        if (mk_seq_hit(run.data(), len, lane, sq.data(), (int)L))
          mk_cover_occurrence(cover.data(), lane, sq.data(), (int)L, [](unsigned* word, unsigned bits) { *word |= bits; });
    }
    int in_round = 0;
    for (int lane = 0; lane < kPhLanes; ++lane) {  // the ballot's prefix count is the lane order
      const unsigned m = lane < len ? mk_mark(run[(size_t)lane], q.loose, cover[(size_t)lane]) : 0u;
      if (!m) continue;
      const int at = n_marks + in_round++;
      if (at < kMkMaxMarks) {
        const int s = mk_slot_of(m);
        m_pos[(size_t)at] = (int)(base - begin) + lane, m_slot[(size_t)at] = (unsigned char)s, kept_slots |= 1u << s;
      }
    }
    n_marks += in_round;
    std::vector<unsigned> next((size_t)kMkStage);
    for (int i = 0; i < kMkStage; ++i) next[(size_t)i] = mk_cover_carry(cover.data(), i);
    cover = next;
  }
  most_marks = std::max<long long>(most_marks, n_marks);
  const int n_kept = std::min(n_marks, kMkMaxMarks);
  double lane_best[kPhLanes];
  int lane_i[kPhLanes];
  for (int lane = 0; lane < kPhLanes; ++lane) lane_best[lane] = 0.0, lane_i[lane] = -1;
  for (int a0 = 0; a0 < n_kept; a0 += kPhLanes)
    for (int lane = 0; lane < kPhLanes; ++lane) {
      const int i = a0 + lane;
      if (i >= n_kept) continue;
      unsigned bits;
      int e;
      (void)mk_window_scan(m_pos.data(), m_slot.data(), n_kept, i, W, doc_len, &bits, &e);
      const double sc = mk_score(bits, q.w.data());
      if (mk_better(sc, i, lane_best[lane], lane_i[lane])) lane_best[lane] = sc, lane_i[lane] = i;
    }
  for (int s = 1; s < kPhLanes; s <<= 1) {  // the butterfly: both partners keep the better of the two
    double nb[kPhLanes];
    int ni[kPhLanes];
    for (int lane = 0; lane < kPhLanes; ++lane) {
      const int o = lane ^ s;
      const bool take = mk_better(lane_best[o], lane_i[o], lane_best[lane], lane_i[lane]);
      nb[lane] = take ? lane_best[o] : lane_best[lane], ni[lane] = take ? lane_i[o] : lane_i[lane];
    }
    std::copy(nb, nb + kPhLanes, lane_best), std::copy(ni, ni + kPhLanes, lane_i);
  }
  for (int lane = 1; lane < kPhLanes; ++lane)
    CHECK(lane_i[lane] == lane_i[0] && std::memcmp(&lane_best[lane], &lane_best[0], 8) == 0, "the lanes disagree on the best window");
  Result r{};
  const int best_i = lane_i[0];
  r.win[0] = 0, r.win[1] = (int)std::min<long long>(doc_len, W), r.win[2] = 0, r.win[3] = n_marks;
  if (best_i >= 0) {
    r.win[0] = m_pos[(size_t)best_i];
    r.win[2] = mk_window_scan(m_pos.data(), m_slot.data(), n_kept, best_i, W, doc_len, &r.slots[0], &r.win[1]);
  }
  r.score = best_i >= 0 ? lane_best[0] : 0.0;
  r.slots[1] = kept_slots, r.status = n_marks > kMkMaxMarks;
  r.marks.assign((size_t)cap * 2, -1);
  for (int lane = 0; lane < cap; ++lane)
    if (lane < r.win[2]) r.marks[2 * (size_t)lane] = m_pos[(size_t)(best_i + lane)], r.marks[2 * (size_t)lane + 1] = m_slot[(size_t)(best_i + lane)];
  return r;
}

Query make_query(Rng& r, int n_terms) {
  Query q;
  const int n_slots = 1 + (int)r.below(6);
  for (int t = 0; t < n_terms; ++t)
    if (r.below(3) != 0) q.terms.push_back(t), q.slot.push_back((int)r.below(n_slots) + (r.below(40) == 0 ? 31 - n_slots : 0));
  q.terms = std::vector<int>(q.terms.begin(), q.terms.end()), q.slot = std::vector<int>(q.slot.begin(), q.slot.end());
  for (int s = 0; s < 32; ++s) q.w.push_back((double)r.below(1000) / 997.0 + (s % 3) * 0.1);
  q.loose = (unsigned)r.below(1L << n_slots);
  const long n_seq = r.below(4);
  for (long s = 0; s < n_seq; ++s) {
    const long L = r.below(9) == 0 ? kPhMaxLen : 2 + r.below(3);
    std::vector<int> sq;
    for (long j = 0; j < L; ++j) sq.push_back((int)r.below(n_slots));
    if (r.below(15) == 0) sq[0] = 32;  // never occurs
    q.seqs.push_back(std::vector<int>(sq.begin(), sq.end()));
  }
  if (r.below(12) == 0) q.seqs.push_back(std::vector<int>(17, 0));  // a length the rule does not define
  return q;
}

void family(int n_terms, uint64_t seed) {
  Rng r{seed};
  const long special[] = {0, 1, 63, 64, 65, 79, 128, 1500, 2, 78, 80, 127, 129, 143, 144, 1100};
  std::vector<std::vector<int>> docs;
  for (long d = 0; d < 28; ++d) {
    const long len = d < 16 ? special[d] : r.below(300);
    std::vector<int> seq;
    for (long i = 0; i < len; ++i) seq.push_back((int)r.below(n_terms));
    docs.push_back(seq);
  }
  std::vector<int> st;
  std::vector<long long> dp{0};
  for (auto& d : docs) st.insert(st.end(), d.begin(), d.end()), dp.push_back((long long)st.size());
  const std::vector<int> stream(st.begin(), st.end());
  long pairs = 0, truncated = 0;
  for (int qi = 0; qi < 12; ++qi) {
    const Query q = make_query(r, n_terms);
    const int Ws[] = {1, 2, 5, 48, 64, 65, 700, kMkMaxWindow};
    for (size_t d = 0; d < docs.size(); ++d) {
      const int W = Ws[(qi + d) % 8], cap = (int)((qi * 7 + d * 5) % 65);
      const Result want = naive(docs[d], q, W, cap), got = wave(stream, dp[d], dp[d + 1], q, W, cap);
      CHECK(same(want, got), "terms=%d query %d document %zu (len %zu, W %d, cap %d): win %d %d %d %d / %d %d %d %d, score %.17g / %.17g",
            n_terms, qi, d, docs[d].size(), W, cap, want.win[0], want.win[1], want.win[2], want.win[3], got.win[0], got.win[1],
            got.win[2], got.win[3], want.score, got.score);
      ++pairs, truncated += got.status;
    }
  }
  std::printf("marks terms=%d: %ld pairs, %ld past the cap, longest staged run %lld, most marks %lld\n", n_terms, pairs, truncated,
              longest_run, most_marks);
  if (failures == 0) std::printf("family ok\n");
}

Result one(const std::vector<int>& before, const std::vector<int>& doc, const std::vector<int>& after, const Query& q, int W, int cap) {
  std::vector<int> st(before);
  st.insert(st.end(), doc.begin(), doc.end()), st.insert(st.end(), after.begin(), after.end());
  const std::vector<int> stream(st.begin(), st.end());
  const Result got = wave(stream, (long long)before.size(), (long long)(before.size() + doc.size()), q, W, cap);
  CHECK(same(got, naive(doc, q, W, cap)), "a written-out case differs from the naive scan");
  return got;
}

void written_out() {
  const int a = 0, b = 1, c = 2, x = 9;
  std::vector<double> w(32, 1.0);
  w[0] = 0.1, w[1] = 0.2, w[2] = 0.3;
  const Query ab{{a, b}, {0, 1}, w, 0u, {{0, 1}}};       // both slots are phrase members only
  const Query ab_a{{a, b}, {0, 1}, w, 1u, {{0, 1}}};     // a is loose as well
  const Query abc{{a, b, c}, {0, 1, 2}, w, 7u, {}};
  Result r = one({}, {x, a, x, b, x}, {}, ab, 48, 4);
  CHECK(r.win[3] == 0 && r.win[0] == 0 && r.win[1] == 5 && r.score == 0.0 && r.slots[1] == 0u, "phrase-only slots standing alone");
  r = one({}, {x, a, x, b, x}, {}, ab_a, 48, 4);
  CHECK(r.win[3] == 1 && r.win[0] == 1 && r.marks[0] == 1 && r.marks[1] == 0 && r.marks[2] == -1, "the loose slot alone");
  r = one({x, a}, {b, x, a}, {b, x}, ab, 48, 4);
  CHECK(r.win[3] == 0, "a phrase never reaches into a neighbour");
  r = one({}, {x, x, a, b}, {b}, ab, 48, 4);
  CHECK(r.win[3] == 2 && r.win[0] == 2 && r.win[1] == 4 && r.slots[0] == 3u, "a phrase ending at the document's end");
  {  // a phrase over the round edge: positions 60 .. 66 of 79
    std::vector<int> doc(79, x);
    Query seven{{0, 1, 2, 3, 4, 5, 6}, {0, 1, 2, 3, 4, 5, 6}, w, 0u, {{0, 1, 2, 3, 4, 5, 6}}};
    for (int j = 0; j < 7; ++j) doc[(size_t)(60 + j)] = j;
    r = one({}, doc, {}, seven, 7, 64);
    CHECK(r.win[3] == 7 && r.win[0] == 60 && r.win[1] == 67 && r.win[2] == 7 && r.marks[12] == 66 && r.marks[13] == 6, "the round edge");
  }
  r = one({}, {c, x, b, x, a, x, x, x, a, b, c}, {}, abc, 3, 8);
  const double want = 0.1 + 0.2 + 0.3;  // in ascending slot order; 0.3 + 0.2 + 0.1 has other bits
  CHECK(r.win[0] == 8 && r.win[2] == 3 && std::memcmp(&r.score, &want, 8) == 0 && (0.3 + 0.2) + 0.1 != want, "the addition order");
  r = one({}, {a, x, x, a, x, x, a}, {}, abc, 2, 8);
  CHECK(r.win[0] == 0 && r.win[2] == 1 && r.win[3] == 3, "equal windows go to the earlier");
  r = one({}, std::vector<int>(1500, a), {}, abc, 4096, 64);
  CHECK(r.status == 1 && r.win[3] == 1500 && r.win[0] == 0 && r.win[1] == 1500 && r.win[2] == kMkMaxMarks && r.marks[126] == 63, "past the cap");
  r = one({}, {}, {a}, abc, 5, 3);
  CHECK(r.win[1] == 0 && r.win[3] == 0 && r.status == 0, "an empty document");
  if (failures == 0) std::printf("written-out ok\n");
}

void validation() {
  const int64_t docs[] = {0, -1, 3, 2}, docs_bad[] = {0, -2, 3, 2}, docs_big[] = {0, 4, 3, 2};
  const int64_t mp[] = {0, 2, 3}, mp_off[] = {1, 2, 3}, mp_down[] = {0, 3, 2};
  const int32_t mt[] = {1, 5, 0}, mt_same[] = {5, 5, 0}, mt_big[] = {1, 10, 0}, mt_neg[] = {-1, 5, 0};
  const int32_t ms[] = {0, 31, 4}, ms_big[] = {0, 32, 4};
  double w[64];
  for (double& v : w) v = 0.5;
  double w_inf[64], w_nan[64];
  std::copy(w, w + 64, w_inf), std::copy(w, w + 64, w_nan);
  w_inf[40] = std::numeric_limits<double>::infinity(), w_nan[3] = std::nan("");
  const uint32_t loose[] = {1u, 0xFFFFFFFFu};
  const int64_t sp[] = {0, 1, 2}, so[] = {0, 2, 18}, so_one[] = {0, 1, 18}, so_long[] = {0, 2, 19}, so_down[] = {0, 2, 1};
  int32_t ss[19];
  for (int32_t& v : ss) v = 3;
  int32_t ss_bad[19];
  std::copy(ss, ss + 19, ss_bad), ss_bad[7] = 32;
  auto v = [&](const int64_t* d, const int64_t* mp_, const int32_t* mt_, const int32_t* ms_, const double* w_, const int64_t* so_,
               const int32_t* ss_) { return mk_validate(d, 2, 2, 2, mp_, mt_, ms_, w_, loose, sp, so_, ss_, 10, 4); };
  CHECK(v(docs, mp, mt, ms, w, so, ss) == kPhValid, "valid operands");
  CHECK(v(docs_bad, mp, mt, ms, w, so, ss) == kMkDoc && v(docs_big, mp, mt, ms, w, so, ss) == kMkDoc, "a hit id outside [-1, n_docs)");
  CHECK(v(docs, mp_off, mt, ms, w, so, ss) == kMkPtr && v(docs, mp_down, mt, ms, w, so, ss) == kMkPtr, "mk_ptr");
  CHECK(v(docs, mp, mt_same, ms, w, so, ss) == kMkTermOrder, "terms not strictly ascending");
  CHECK(v(docs, mp, mt_big, ms, w, so, ss) == kMkTerm && v(docs, mp, mt_neg, ms, w, so, ss) == kMkTerm, "a term outside the vocabulary");
  CHECK(v(docs, mp, mt, ms_big, w, so, ss) == kMkSlot && v(docs, mp, mt, ms, w, so, ss_bad) == kMkSlot, "a slot outside 0 .. 31");
  CHECK(v(docs, mp, mt, ms, w_inf, so, ss) == kMkWeight && v(docs, mp, mt, ms, w_nan, so, ss) == kMkWeight, "a weight that is not finite");
  CHECK(v(docs, mp, mt, ms, w, so_one, ss) == kMkSeqLength && v(docs, mp, mt, ms, w, so_long, ss) == kMkSeqLength, "sequence lengths");
  CHECK(v(docs, mp, mt, ms, w, so_down, ss) == kMkPtr, "sq_off");
  CHECK(v(nullptr, mp, mt, ms, w, so, ss) == kPhNull && v(docs, nullptr, mt, ms, w, so, ss) == kPhNull &&
        v(docs, mp, nullptr, ms, w, so, ss) == kPhNull && v(docs, mp, mt, ms, nullptr, so, ss) == kPhNull &&
        v(docs, mp, mt, ms, w, so, nullptr) == kPhNull, "null operands");
  const int64_t zero[] = {0};
  CHECK(mk_validate(nullptr, 0, 5, 5, zero, nullptr, nullptr, nullptr, nullptr, zero, zero, nullptr, 10, 4) == kPhValid, "no query reads nothing");
  CHECK(mk_validate(docs, -1, 2, 2, mp, mt, ms, w, loose, sp, so, ss, 10, 4) == kPhSizes &&
        mk_validate(docs, 2, 2, 1, mp, mt, ms, w, loose, sp, so, ss, 10, 4) == kPhSizes, "sizes");
  for (int e : {(int)kMkPtr, (int)kMkTermOrder, (int)kMkTerm, (int)kMkSlot, (int)kMkSeqLength, (int)kMkWeight, (int)kMkDoc})
    CHECK(std::string(mk_error_text(e)) != "ok", "an error without words");
  // the table: a slot outside 0 .. 31 fills nothing; the first and the last of 3 000 members and what lies beside them
  std::vector<int> big, slot(3000, 7);
  for (int i = 0; i < 3000; ++i) big.push_back(10 + 2 * i);
  const MkTable T{big.data(), slot.data(), 3000};
  CHECK(mk_token_mask(10, T) == 1u << 7 && mk_token_mask(10 + 2 * 2999, T) == 1u << 7, "the edges of 3 000 members");
  for (int t : {9, 11, 10 + 2 * 2999 + 1, 10 + 2 * 3000, -5}) CHECK(mk_token_mask(t, T) == 0u, "beside the members");
  const int one_t[] = {4}, bad_s[] = {32};
  CHECK(mk_token_mask(4, MkTable{one_t, bad_s, 1}) == 0u && mk_token_mask(4, MkTable{nullptr, nullptr, 0}) == 0u, "an undefined slot, an empty table");
  CHECK(mk_run_len(0, 1000) == kMkStage && kMkStage == 79 && mk_run_len(10, 12) == 2 && mk_run_len(64, 128) == 64, "run lengths");
  if (failures == 0) std::printf("validate ok\n");
}

}  // namespace

int main() {
  for (int n_terms : {2, 4, 9}) family(n_terms, 500 + (uint64_t)n_terms);
  written_out();
  validation();
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("marks rule ok\n");
  return 0;
}
