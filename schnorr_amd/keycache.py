"""KeyCache: a registered key set run as a key cache, with the census closing the loop (include/dsv.h, "key cache
census").  A small host policy — the demonstration of how admission (KeySet.append), eviction
(KeySet.replace) and the census fit together, not a second engine:

    cache = KeyCache("single", 4096)
    cache.verify_open_dev(u, R, PK, m, ok, workspace)   # the set's open-set verify + the census, one stream
    ...                                                  # (more batches)
    cache.maintain()                                     # between batches: admit the busy keys, evict the idle ones

Scores are exponentially decayed hit counts: maintain() halves them and adds the hits since the last call.  A missed
key is admitted while there is room, and afterwards in the place of the lowest-score key whose score is below the
number of items the missed key carried."""
import numpy as np

from . import engine as E


class KeyCache:
    def __init__(self, scheme, capacity, device="cuda:0"):
        import torch

        self.scheme, self.capacity, self.device = scheme, int(capacity), torch.device(device)
        self.ks = E.KeySet.reserved(scheme, self.capacity)
        self.scores = np.zeros(self.capacity, dtype=np.float64)
        self.refused = set()  # key bytes that came back with key_ok = 0: never offered again
        self._hits = torch.zeros(max(self.capacity, 1), dtype=torch.int32, device=self.device)
        self._batch = None    # the latest batch's key columns and report tensors, until maintain() reads them

    def close(self):
        self.ks.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def verify_open_dev(self, *args, misses=None, stream=None):
        """(u, R[, Rp], key_a[, key_b], m, ok, workspace) as KeySet.verify_open_dev (var-generator sets:
        verify_vargen_open_dev) takes them: enqueues that call, then the census over the same key columns on the
        same stream; does not synchronise.  The key columns must stay as they are until maintain() has read them."""
        import torch

        open_dev = self.ks.verify_vargen_open_dev if self.scheme == "vargen" else self.ks.verify_open_dev
        open_dev(*args, misses=misses, stream=stream)
        keys = self.ks._by_value(args[:-2], "verify_open_dev")[2]
        n = keys[0].shape[0]
        b = self._batch
        if b is None or b["rep"].shape[0] < n:
            new = lambda count, dtype=torch.int32: torch.empty(count, dtype=dtype, device=self.device)
            b = dict(rep=new(n), count=new(n), totals=new(4),
                     ws=new(E.keyset_census_workspace_bytes(n), torch.uint8))
        b.update(keys=keys, n=n, stream=stream if stream is not None else torch.cuda.current_stream(self.device))
        self._batch = b
        self.ks.census_dev(*keys, None, self._hits, b["rep"][:n], b["count"][:n], b["totals"], b["ws"],
                           stream=b["stream"])

    def _offer(self, rows, counts, indices):
        """registers rows[j] (key bytes, one row per key) at indices[j] (None: appended) and scores them; a key that
        comes back invalid is remembered and its place scored 0"""
        two = self.scheme != "single"
        cols = [np.ascontiguousarray(rows[:, :64])] + ([np.ascontiguousarray(rows[:, 64:])] if two else [])
        if indices is None:
            first = self.ks.append(*cols)
            indices = np.arange(first, first + len(rows))
        else:
            self.ks.replace(indices, *cols)
        key_ok = self.ks.key_ok()
        for j, at in enumerate(indices):
            self.scores[at] = counts[j] if key_ok[at] else 0.0
            if not key_ok[at]:
                self.refused.add(rows[j].tobytes())

    def maintain(self):
        """Waits for the latest verify_open_dev's stream, folds the hits since the last call into the scores and
        acts on that batch's report: appends the busiest missed keys while there is room, then replaces the
        lowest-score keys whose score is below the candidate's count.  Returns dict(appended, replaced, refused).

        It calls KeySet.replace and so inherits its duties: no stream of the device may be capturing, and no graph
        that holds the set may be replayed, while it runs; it blocks and quiesces the device."""
        import torch

        out = dict(appended=0, replaced=0, refused=len(self.refused))
        b = self._batch
        if b is None or b["keys"] is None:
            return out
        b["stream"].synchronize()
        self.scores = self.scores / 2
        self.scores[:self.capacity] += self._hits[:self.capacity].cpu().numpy().astype(np.float64)
        self._hits.zero_()
        d = int(b["totals"][0].item())
        rep = b["rep"][:d].cpu().numpy().view(np.uint32).astype(np.int64)
        count = b["count"][:d].cpu().numpy().view(np.uint32).astype(np.int64)
        order = np.lexsort((rep, -count))  # count descending, then representative ascending
        rep, count = rep[order], count[order]
        at = torch.from_numpy(rep).to(self.device)
        rows = np.hstack([c.index_select(0, at).cpu().numpy() for c in b["keys"]]) if d else np.zeros((0, 64), np.uint8)
        keep = [j for j in range(d) if rows[j].tobytes() not in self.refused]
        rows, count = rows[keep], count[keep]
        b["keys"] = None  # the report is spent; its tensors serve the next batch
        room = self.capacity - self.ks.k
        if room and len(rows):
            m = min(room, len(rows))
            self._offer(rows[:m], count[:m], None)
            out["appended"] = m
            rows, count = rows[m:], count[m:]
        victims = np.argsort(self.scores[:self.ks.k], kind="stable")
        m = 0
        while m < min(len(rows), len(victims)) and self.scores[victims[m]] < count[m]:
            m += 1
        if m:
            self._offer(rows[:m], count[:m], victims[:m].astype(np.uint32))
            out["replaced"] = m
        out["refused"] = len(self.refused)
        return out
