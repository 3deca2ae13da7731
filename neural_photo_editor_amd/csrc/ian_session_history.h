// ian_session_history.h -- the bookkeeping of one edit session's undo history (ian_session_mark / ian_session_undo).
// Plain C++: no HIP, no handle types.  The same specification is npe_ops.SessionHistory in Python; tests/session_history_main.cpp
// runs this header on the CPU against it.
//
// A session's history is a list of saved states E[0..len-1] and a cursor c, 0 <= c <= len.  c == len: the live state is not in the
// list; c < len: the live state is E[c].  The entries live in a ring of depth + 1 physical slots, entry k in slot
// (base + k) % (depth + 1).  Every function returns physical slots; what is in a slot is the caller's business.
//   invariant: c == len implies len <= depth; c < len implies len <= depth + 1.  So at most `depth` steps can be undone, and the one
//   slot beyond them holds the tip that the first undo saves.
#ifndef IAN_SESSION_HISTORY_H
#define IAN_SESSION_HISTORY_H

namespace ian {

constexpr int SESSION_HISTORY_MAX_DEPTH = 64;

struct SessionHistory {
  int base = 0;   // physical slot of E[0]
  int len = 0;
  int cur = 0;    // the cursor c
};

inline int session_history_slot(const SessionHistory& H, int depth, int k) { return (H.base + k) % (depth + 1); }
inline void session_history_drop_oldest(SessionHistory& H, int depth) {
  H.base = (H.base + 1) % (depth + 1);
  --H.len;
  if (H.cur > 0) --H.cur;
}
inline int session_history_undoable(const SessionHistory& H) { return H.cur; }
inline int session_history_redoable(const SessionHistory& H) { return H.cur < H.len ? H.len - 1 - H.cur : 0; }

// "a stroke begins": the redo tail goes, the oldest entry too when the list is full, the live state becomes the last entry.
// -> the slot to save the live state into
inline int session_history_mark(SessionHistory& H, int depth) {
  if (H.cur < H.len) H.len = H.cur;
  if (H.len == depth) {
    H.cur = H.len;   // c == len here: dropping E[0] moves both
    session_history_drop_oldest(H, depth);
  }
  const int slot = session_history_slot(H, depth, H.len);
  ++H.len;
  H.cur = H.len;
  return slot;
}

// 1 <= k <= undoable.  The first undo from the tip saves the live state behind the list (*save = its slot, otherwise -1), so that
// redo can come back to it.  -> the slot to load
inline int session_history_undo(SessionHistory& H, int depth, int k, int* save) {
  *save = -1;
  if (H.cur == H.len) {
    *save = session_history_slot(H, depth, H.len);
    ++H.len;
  }
  H.cur -= k;
  return session_history_slot(H, depth, H.cur);
}

// 1 <= k <= redoable -> the slot to load
inline int session_history_redo(SessionHistory& H, int depth, int k) {
  H.cur += k;
  return session_history_slot(H, depth, H.cur);
}

// the session's latent was written by something other than undo / redo: the redo tail goes, the state the user came back to stays
// an undo target.  With depth + 1 entries before the cursor the oldest goes, which keeps the invariant above.
inline void session_history_edited(SessionHistory& H, int depth) {
  if (H.cur >= H.len) return;
  H.len = H.cur + 1;
  H.cur = H.len;
  if (H.len > depth) session_history_drop_oldest(H, depth);
}

inline void session_history_clear(SessionHistory& H) { H = SessionHistory{}; }

}  // namespace ian

#endif
