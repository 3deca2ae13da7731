// Stand-alone driver of csrc/ian_session_record.h for tests/test_sessions_record_host.py: reads the pool's layout
// "num_latents scale local depth body_bytes" and then one command per line from stdin, and prints one line per command:
//   p BYTES                    -> session_record_pad(BYTES)
//   r BASE DEPTH K             -> session_record_ring_slot(BASE, DEPTH, K)
//   m MAGIC FORMAT NUM_LATENTS SCALE LOCAL DEPTH HAS_SOURCE LOCAL_FLAGS HIST_LEN HIST_CUR BODY_BYTES R0 R1 R2 R3
//                              -> "ok", or the name of the field session_record_check refuses
#include <cstdint>
#include <cstdio>

#include "ian_session_record.h"

struct Meta {   // ian_session_meta's members (include/ian.h)
  uint32_t magic;
  int32_t format, num_latents, scale, local, depth, has_source, local_flags, hist_len, hist_cur;
  int64_t body_bytes;
  int32_t reserved[4];
};

int main() {
  static_assert(sizeof(Meta) == 64, "the meta block is 64 bytes");
  ian::SessionRecordLayout L;
  if (std::scanf("%d %d %d %d %lld", &L.num_latents, &L.scale, &L.local, &L.depth, &L.body_bytes) != 5) return 2;
  char op = 0;
  while (std::scanf(" %c", &op) == 1) {
    if (op == 'p') {
      unsigned long long b = 0;
      if (std::scanf("%llu", &b) != 1) return 2;
      std::printf("%llu\n", (unsigned long long)ian::session_record_pad((size_t)b));
    } else if (op == 'r') {
      int base = 0, depth = 0, k = 0;
      if (std::scanf("%d %d %d", &base, &depth, &k) != 3 || depth < 0 || base < 0 || k < 0) return 2;
      std::printf("%d\n", ian::session_record_ring_slot(base, depth, k));
    } else if (op == 'm') {
      Meta m;
      long long magic = 0, bb = 0;
      if (std::scanf("%lld %d %d %d %d %d %d %d %d %d %lld %d %d %d %d", &magic, &m.format, &m.num_latents, &m.scale, &m.local, &m.depth,
                     &m.has_source, &m.local_flags, &m.hist_len, &m.hist_cur, &bb, &m.reserved[0], &m.reserved[1], &m.reserved[2],
                     &m.reserved[3]) != 15)
        return 2;
      m.magic = (uint32_t)magic;
      m.body_bytes = bb;
      const ian::SessionRecordRefusal r = ian::session_record_check(m, L);
      std::printf("%s\n", r.field ? r.field : "ok");
    } else {
      return 2;
    }
  }
  return 0;
}
