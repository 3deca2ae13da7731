// Stand-alone driver of csrc/ian_session_history.h for tests/test_sessions_history_host.py: reads "depth" and then one operation
// per line from stdin (m | u K | r K | e | c) and prints, per operation, the physical slots the header returns and the counters:
//   m SLOT U R | u SAVE LOAD U R | r LOAD U R | e U R | c U R | x U R (more steps than there are: refused, nothing moves)
#include <cstdio>

#include "ian_session_history.h"

int main() {
  int depth = 0;
  if (std::scanf("%d", &depth) != 1 || depth < 1 || depth > ian::SESSION_HISTORY_MAX_DEPTH) return 2;
  ian::SessionHistory H;
  char op = 0;
  while (std::scanf(" %c", &op) == 1) {
    int k = 0;
    if ((op == 'u' || op == 'r') && std::scanf("%d", &k) != 1) return 2;
    if (op == 'm') {
      std::printf("m %d", ian::session_history_mark(H, depth));
    } else if (op == 'u' && k >= 1 && k <= ian::session_history_undoable(H)) {
      int save = -1;
      const int load = ian::session_history_undo(H, depth, k, &save);
      std::printf("u %d %d", save, load);
    } else if (op == 'r' && k >= 1 && k <= ian::session_history_redoable(H)) {
      std::printf("r %d", ian::session_history_redo(H, depth, k));
    } else if (op == 'e') {
      ian::session_history_edited(H, depth);
      std::printf("e");
    } else if (op == 'c') {
      ian::session_history_clear(H);
      std::printf("c");
    } else if (op == 'u' || op == 'r') {
      std::printf("x");
    } else {
      return 2;
    }
    std::printf(" %d %d\n", ian::session_history_undoable(H), ian::session_history_redoable(H));
  }
  return 0;
}
