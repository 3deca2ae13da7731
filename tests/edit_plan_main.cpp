// Stand-alone driver of csrc/ian_edit_plan.h for tests/test_sessions_plan_host.py, built under AddressSanitizer and UBSan.  One case per
// run:   edit_plan pass save tips own_rows v c0 c1 ...     the counts as an array
//        edit_plan pass save tips own_rows u n c           n items of count c, as the brush and the clone give them (one word, stride 0)
// The plan, the table and every pass's steps are checked against the brute-force model "for k: the items with more than k points,
// split into passes of `pass`"; every buffer is a heap block of exactly the size the header promises.  Prints
// "ok words=W middles=M blends=B reforwards=R resident=0|1", or the first difference and exit status 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ian_edit_plan.h"

#define CHECK(cond, ...)                          \
  do {                                            \
    if (!(cond)) {                                \
      printf("line %d: %s: ", __LINE__, #cond);   \
      printf(__VA_ARGS__);                        \
      printf("\n");                               \
      return 1;                                   \
    }                                             \
  } while (0)

int main(int argc, char** argv) {
  using namespace ian;
  if (argc < 7) return 2;
  const int pass = atoi(argv[1]);
  const bool save = atoi(argv[2]) != 0, tips = atoi(argv[3]) != 0, own = atoi(argv[4]) != 0, uniform = !strcmp(argv[5], "u");
  if (pass < 1 || (uniform ? argc != 8 : strcmp(argv[5], "v") != 0)) return 2;
  std::vector<int> cnt;   // the model's copy
  if (uniform) cnt.assign((size_t)atoi(argv[6]), atoi(argv[7]));
  else for (int i = 6; i < argc; ++i) cnt.push_back(atoi(argv[i]));
  const int n = (int)cnt.size();
  for (int i = 0; i < n; ++i)
    if (cnt[i] < 1 || cnt[i] > EDIT_MAX_STEPS || (i > 0 && cnt[i] > cnt[i - 1])) return 2;
  // what the header reads: exactly the words it may
  int32_t* words = new int32_t[uniform ? 1 : (size_t)n];
  for (int i = 0; i < (uniform ? 1 : n); ++i) words[i] = cnt[i];
  const EditPlan P = edit_plan(n, words, uniform ? 0 : 1, own);

  // ---- the rows: step k's are the items with more than k points, after those of the steps before it
  CHECK(P.n == n && P.steps == cnt[0], "n %d steps %d", P.n, P.steps);
  int before = 0;
  for (int k = 0; k <= P.steps; ++k) {
    CHECK(P.rows[k] == (own ? before : 0), "rows[%d] = %d, the model has %d", k, P.rows[k], own ? before : 0);
    for (int i = 0; i < n; ++i) before += cnt[i] > k;
  }
  CHECK(P.nrows == (own ? before : n), "nrows %d", P.nrows);

  // ---- the table: the columns in order, none overlapping, ending exactly at the word count
  const EditTable L = edit_table(P, save, tips);
  const size_t un = (size_t)n;
  const size_t at[6] = {L.ids, L.save, L.seed, L.rows, L.items, L.tips};
  const size_t width[6] = {un, save ? un : 0, 3 * un, own ? (size_t)P.steps + 1 : 0, (size_t)EDIT_ROW_WORDS * P.nrows, tips ? un : 0};
  CHECK(L.has_save == save && L.has_tips == tips, "flags");
  char* cell = new char[L.words]();
  size_t sum = 0;
  for (int c = 0; c < 6; ++c) {
    CHECK(at[c] == sum, "column %d at %zu, after %zu words", c, at[c], sum);
    for (size_t w = 0; w < width[c]; ++w) CHECK(cell[at[c] + w]++ == 0, "column %d overlaps at word %zu", c, at[c] + w);
    sum += width[c];
  }
  CHECK(sum == L.words, "%zu words, the columns have %zu", L.words, sum);
  delete[] cell;

  // ---- the steps of every pass
  std::vector<int> next((size_t)n, 0), blended((size_t)n, 0);
  char* row_used = new char[(size_t)P.nrows]();
  int middles = 0, blends = 0, reforwards = 0;
  for (int off = 0; off < n; off += pass) {
    const int nc = n - off < pass ? n - off : pass;
    int k = 0, expect_act = nc;
    const int rc = edit_pass_steps(P, off, nc, [&](const EditStep& s) -> int {
      CHECK(s.step == k, "pass at %d: step %d where %d is due", off, s.step, k);
      int act = 0, keep = 0;   // the model: this pass's items with more than k, more than k + 1 points
      for (int i = off; i < off + nc; ++i) act += cnt[i] > k, keep += cnt[i] > k + 1;
      CHECK(act > 0 && s.act == act && s.keep == keep && s.act == expect_act, "pass at %d step %d: act %d keep %d, the model has %d %d", off, k, s.act,
            s.keep, act, keep);
      int model_row = off;   // own rows: the rows of the steps before, then this step's items before the pass
      for (int kk = 0; own && kk < k; ++kk)
        for (int i = 0; i < n; ++i) model_row += cnt[i] > kk;
      CHECK(s.row == model_row, "pass at %d step %d: row %d, the model has %d", off, k, s.row, model_row);
      for (int i = off; i < off + s.act; ++i) {   // every (item, step) once and in order, on a row of its own
        CHECK(next[i] == k && k < cnt[i], "item %d runs step %d after %d of its %d", i, k, next[i], cnt[i]);
        ++next[i];
        const int r = s.row + (i - off);
        CHECK(r >= 0 && r < P.nrows, "item %d step %d: row %d of %d", i, k, r, P.nrows);
        if (own) CHECK(row_used[r]++ == 0, "row %d is read twice", r);
        else CHECK(r == i, "item %d reads row %d", i, r);
      }
      ++middles;
      for (int i = off + s.keep; i < off + s.act; ++i) {   // the ones that end here are blended, once, at their last step
        CHECK(cnt[i] == k + 1 && blended[i] == 0, "item %d of %d points is blended after step %d", i, cnt[i], k);
        ++blended[i];
      }
      for (int i = off; i < off + s.keep; ++i) CHECK(cnt[i] > k + 1, "item %d of %d points is kept after step %d", i, cnt[i], k);
      if (s.keep < s.act) ++blends;
      if (s.keep < s.act && s.keep > 0) ++reforwards;   // what edit_passes does with (act, keep): the forward again at batch keep
      expect_act = s.keep;
      ++k;
      return 0;
    });
    CHECK(rc == 0, "a pass ended early");
    CHECK(k == cnt[off] && expect_act == 0, "pass at %d: %d steps for %d points, %d items left", off, k, cnt[off], expect_act);
  }
  for (int i = 0; i < n; ++i) CHECK(next[i] == cnt[i] && blended[i] == 1, "item %d: %d of %d steps, %d blends", i, next[i], cnt[i], blended[i]);
  for (int r = 0; own && r < P.nrows; ++r) CHECK(row_used[r] == 1, "row %d is never read", r);
  // the model's counts: a blend per (pass, distinct count in it), a forward again after each unless the pass has no items before them
  int model_blends = 0, model_reforwards = 0;
  for (int off = 0; off < n; off += pass)
    for (int i = off, first = off; i < off + pass && i < n; ++i) {
      if (i > off && cnt[i] != cnt[i - 1]) first = i;
      if (i + 1 == n || i + 1 == off + pass || cnt[i + 1] != cnt[i]) {
        ++model_blends;
        model_reforwards += first > off;
      }
    }
  CHECK(blends == model_blends && reforwards == model_reforwards, "%d blends %d reforwards, the model has %d %d", blends, reforwards, model_blends,
        model_reforwards);
  bool same = true;
  for (int i = 1; i < n; ++i) same = same && cnt[i] == cnt[0];
  CHECK(edit_plan_resident(P, pass) == (n <= pass && same), "resident %d", (int)edit_plan_resident(P, pass));
  printf("ok words=%zu middles=%d blends=%d reforwards=%d resident=%d\n", L.words, middles, blends, reforwards, (int)edit_plan_resident(P, pass));
  delete[] row_used;
  delete[] words;
  return 0;
}
