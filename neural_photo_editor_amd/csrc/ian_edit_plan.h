// ian_edit_plan.h -- the calls that run brush steps on edit sessions (ian_session_brush, _clone, _stroke and their forms):
// which item runs which step in which pass, and where the parts of the call's one uploaded table lie.  Host only, no HIP and no handle:
// edit_passes (ian_rt_session.inc) enqueues what this says, tests/edit_plan_main.cpp holds it to a brute-force model under the sanitizers.
#ifndef IAN_EDIT_PLAN_H_
#define IAN_EDIT_PLAN_H_

#include <cstddef>
#include <cstdint>
namespace ian {
constexpr int EDIT_MAX_STEPS = 64;   // IAN_STROKE_MAX_POINTS, IAN_CLONE_MAX_STEPS
constexpr int EDIT_ROW_WORDS = 7;    // ian_brush_item: c1 r1 c2 r2 loss-kind coef gscale

// n items; item i runs steps 0 .. count(i) - 1, 1 <= count <= EDIT_MAX_STEPS, not increasing with i (cstride 0: one count for all).  So
// the items of a step are a prefix of the array, the ones that end at it the tail of that prefix, and a pass a slice of every step.
// own_rows: every step has its own item rows, one per item that runs it (a stroke); otherwise one row per item serves all its steps
// (a brush event: one step; a clone: `steps` of them).
struct EditPlan {
  int n, steps;                     // steps: item 0's, the most
  const int32_t* counts; int cstride; bool own_rows;
  int nrows;                        // item rows in the table
  int rows[EDIT_MAX_STEPS + 1];     // own_rows: rows[k] = the rows before step k's; otherwise zeros
  int count(int i) const { return counts[(size_t)i * cstride]; }
};
inline EditPlan edit_plan(int n, const int32_t* counts, int cstride, bool own_rows) {
  EditPlan P = {n, counts[0], counts, cstride, own_rows, n, {0}};
  for (int k = 0, act = n; own_rows && k < P.steps; ++k) {
    while (act > 0 && P.count(act - 1) <= k) --act;
    P.nrows = P.rows[k + 1] = P.rows[k] + act;
  }
  return P;
}
// The table, in words: [n ids | n history slots (save) | 3n seed words: colours, or a clone's source | steps + 1 row offsets (own_rows)
// | nrows item rows | n tip indices (tips)].  A column the call does not have is empty: it starts where the next one does.
struct EditTable { size_t ids, save, seed, rows, items, tips, words; bool has_save, has_tips; };
inline EditTable edit_table(const EditPlan& P, bool save, bool tips) {
  const size_t n = (size_t)P.n;
  EditTable T = {0, n, 0, 0, 0, 0, 0, save, tips};
  T.seed = T.save + (save ? n : 0);
  T.rows = T.seed + 3 * n;
  T.items = T.rows + (P.own_rows ? (size_t)P.steps + 1 : 0);
  T.tips = T.items + (size_t)EDIT_ROW_WORDS * P.nrows;
  T.words = T.tips + (tips ? n : 0);
  return T;
}

// One step of the pass of items [off, off + nc): the pass's first `act` items run it, on the item rows from `row`; the first `keep`
// of them have a further step.  The others end here: they are blended now, and when 0 < keep the forward runs again at batch keep.
struct EditStep { int step, row, act, keep; };
template <typename F>
int edit_pass_steps(const EditPlan& P, int off, int nc, F f) {   // f(EditStep) -> 0, or the error that ends the walk
  for (int k = 0, act = nc; act > 0; ++k) {
    int keep = act;
    while (keep > 0 && P.count(off + keep - 1) == k + 1) --keep;
    if (int rc = f(EditStep{k, P.rows[k] + off, act, keep})) return rc;
    act = keep;
  }
  return 0;
}
// after the call the decoder's activations belong to all n items at their new latents: one pass, and every item ran in the last forward
inline bool edit_plan_resident(const EditPlan& P, int pass) { return P.n <= pass && P.count(P.n - 1) == P.steps; }

}  // namespace ian
#endif  // IAN_EDIT_PLAN_H_
