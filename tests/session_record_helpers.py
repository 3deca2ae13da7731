"""What the two test files of saved sessions share (test_sessions_record_host.py, test_gpu_sessions_record.py).  Plain functions."""
import numpy as np

from neural_photo_editor_amd import npe_ops as N

# ian_session_meta without its reserved words, in order
META_FIELDS = ("magic", "format", "num_latents", "scale", "local", "depth", "has_source", "local_flags", "hist_len", "hist_cur", "body_bytes")


def random_session(rs, zl, scale, local, entries, with_source):
    """Random contents of one session in the form EditSessions.read returns, and `entries` history entries (Z, UMASK) or Z."""
    img = lambda: rs.randint(0, 256, (3, 64, 64)).astype(np.uint8)
    f = {"GIM": img(), "IM": img(), "RECON": img(), "ERROR": rs.randn(3, 64, 64).astype(np.float32),
         "Z": rs.randn(zl).astype(np.float32), "MODE": int(rs.randint(0, 2))}
    if scale:
        f["FIELD"], f["FIELD_KIND"] = rs.randn(3, 64, 64).astype(np.float32), int(rs.randint(0, 2))
        if with_source:
            f["SOURCE"] = rs.randint(0, 256, (3, 64 * scale, 64 * scale)).astype(np.uint8)
    if local:
        f["UMASK"], f["LOCAL"] = rs.rand(64, 64), int(rs.randint(0, 4))
    hist = []
    for _ in range(entries):
        z = rs.randn(zl).astype(np.float32)
        hist.append((z, rs.rand(64, 64)) if local else z)
    return f, hist


class Tracker:
    """What the history rings of some sessions hold, kept beside a pool by reading Z and UMASK whenever the pool saves a state:
    npe_ops.SessionHistory per session for the bookkeeping, and per physical slot the rows that went into it."""

    def __init__(self, pool, ids):
        self.pool, self.local = pool, pool.local
        self.H = {i: N.SessionHistory(pool.history_depth) for i in ids}
        self.slots = {i: {} for i in ids}

    def _state(self, i):
        f = self.pool.read(i)
        return (f["Z"], f["UMASK"]) if self.local else f["Z"]

    def mark(self, ids):
        for i in ids:
            self.slots[i][self.H[i].mark()] = self._state(i)
        self.pool.mark(ids)

    def undo(self, ids, steps=1):
        for i in ids:
            save, _ = self.H[i].undo(steps)
            if save >= 0:
                self.slots[i][save] = self._state(i)
        return self.pool.undo(ids, steps)

    def redo(self, ids, steps=1):
        for i in ids:
            self.H[i].redo(steps)
        return self.pool.redo(ids, steps)

    def edited(self, ids):
        for i in ids:
            self.H[i].edited()

    def clear(self, ids):
        for i in ids:
            self.H[i].clear()
            self.slots[i] = {}

    def entries(self, i):
        """The history's entries, oldest first, and its cursor."""
        H = self.H[i]
        return [self.slots[i][H._slot(k)] for k in range(H.len)], H.cur


def expected_record(pool, tracker, sid):
    """(meta, body) of session `sid` by the specification: every readable field through ian_session_read, the history from the rows
    read at each save."""
    f = pool.read(sid)
    entries, cur = tracker.entries(sid) if tracker is not None and pool.history_depth else ([], 0)
    return N.session_record_pack(f, entries, len(f["Z"]), pool.scale, pool.local, pool.history_depth, hist_cur=cur)
