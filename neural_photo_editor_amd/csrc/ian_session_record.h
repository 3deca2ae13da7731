// ian_session_record.h -- the host side of a saved edit session (ian_session_save / ian_session_load): the padding
// rule of the body, the validation of a record's meta block against a pool's layout, and where a history entry goes in a record.
// Plain C++: no HIP, no handle types.  The same specification is npe_ops.session_record_layout / check_session_meta in Python;
// tests/session_record_main.cpp runs this header on the CPU against them.
//
// The meta block is ian_session_meta (include/ian.h); the functions here are templates over it so that this header needs no other.
#ifndef IAN_SESSION_RECORD_H
#define IAN_SESSION_RECORD_H

#include <cstddef>

namespace ian {

constexpr unsigned SESSION_RECORD_MAGIC = 0x534e4149u;   // "IANS"
constexpr int SESSION_RECORD_FORMAT = 1;

// every array of a body starts at a multiple of 16 bytes: a lane of the pack / unpack kernels moves 16 bytes of the body at a time
inline size_t session_record_pad(size_t bytes) { return (bytes + 15) & ~(size_t)15; }

// what a record's body depends on
struct SessionRecordLayout {
  int num_latents = 0;
  int scale = 0;    // 0: no full-resolution reservation
  int local = 0;    // 1: the local reservation
  int depth = 0;    // 0: no history reservation
  long long body_bytes = 0;
};

// Entry k of a history whose first entry sits in physical slot `base` of a ring of depth + 1 slots.  In a record entry k is slot k
// (base 0), which is what makes two saves of the same logical state the same bytes.
inline int session_record_ring_slot(int base, int depth, int k) { return (base + k) % (depth + 1); }

struct SessionRecordRefusal {
  const char* field = nullptr;   // nullptr: the meta is fine
  long long got = 0, want = 0;   // the record's value and, for a layout field, the pool's
  const char* why = "";
};

// A record's meta against the layout of the pool it is to be loaded into; the first field that fails, in this order.
template <class Meta>
SessionRecordRefusal session_record_check(const Meta& m, const SessionRecordLayout& L) {
  auto no = [](const char* f, long long got, long long want, const char* why) {
    SessionRecordRefusal r;
    r.field = f; r.got = got; r.want = want; r.why = why;
    return r;
  };
  if (m.magic != SESSION_RECORD_MAGIC) return no("magic", (long long)m.magic, (long long)SESSION_RECORD_MAGIC, "not a session record");
  if (m.format != SESSION_RECORD_FORMAT) return no("format", m.format, SESSION_RECORD_FORMAT, "a format this library does not read");
  const char* layout = "the record comes from another pool layout (layouts must match exactly)";
  if (m.num_latents != L.num_latents) return no("num_latents", m.num_latents, L.num_latents, layout);
  if (m.scale != L.scale) return no("scale", m.scale, L.scale, layout);
  if (m.local != L.local) return no("local", m.local, L.local, layout);
  if (m.depth != L.depth) return no("depth", m.depth, L.depth, layout);
  if (m.body_bytes != L.body_bytes) return no("body_bytes", m.body_bytes, L.body_bytes, layout);
  if (m.local_flags < 0 || m.local_flags > 3) return no("local_flags", m.local_flags, 3, "outside 0..3 (bit 0 = local, bit 1 = dampen)");
  if (m.local_flags != 0 && !L.local) return no("local_flags", m.local_flags, 0, "flags in a layout without the local reservation");
  if (m.has_source < 0 || m.has_source > 1) return no("has_source", m.has_source, 1, "outside 0..1");
  if (m.has_source && L.scale == 0) return no("has_source", m.has_source, 0, "a source at scale 0");
  // ian_session_history.h: 0 <= cur <= len; cur == len implies len <= depth; otherwise len <= depth + 1
  if (m.hist_len < 0) return no("hist_len", m.hist_len, 0, "negative");
  if (m.hist_cur < 0 || m.hist_cur > m.hist_len) return no("hist_cur", m.hist_cur, m.hist_len, "the cursor is outside 0..hist_len");
  if (L.depth == 0 && m.hist_len != 0) return no("hist_len", m.hist_len, 0, "entries in a layout without a history");
  if (m.hist_cur == m.hist_len && m.hist_len > L.depth) return no("hist_len", m.hist_len, L.depth, "more entries than the depth with the cursor at the tip");
  if (m.hist_len > L.depth + 1) return no("hist_len", m.hist_len, L.depth + 1, "more entries than the ring has slots");
  for (int k = 0; k < 4; ++k)
    if (m.reserved[k] != 0) return no("reserved", m.reserved[k], 0, "a reserved word is not zero");
  return SessionRecordRefusal{};
}

}  // namespace ian

#endif
