"""Independent oracle of the rolling episode window (``TrainConfig.ep_window``), written from its specification, not from
``ops/ep_monitor.py``: the double loop over steps and envs in plain Python with ``np.float32`` adds, and the summary in
numpy fp64.

State: ``cur_ret[N]`` fp32 / ``cur_len[N]`` int32 (the unfinished episode of each env), ``ring_ret[K]`` fp32 /
``ring_len[K]`` int32, ``total`` (episodes ever finished). Slot ``total mod K`` is written next."""
import numpy as np

SUMMARY = ("filled", "total", "ret_mean", "ret_std", "ret_min", "ret_max", "len_mean", "new", "new_ret_mean",
           "new_len_mean")


class EpMonitorOracle:
    def __init__(self, N, K):
        self.N, self.K = int(N), int(K)
        self.cur_ret = np.zeros(N, dtype=np.float32)
        self.cur_len = np.zeros(N, dtype=np.int32)
        self.ring_ret = np.zeros(K, dtype=np.float32)
        self.ring_len = np.zeros(K, dtype=np.int32)
        self.total = 0
        self.summary = dict.fromkeys(SUMMARY, 0.0)

    def update(self, rewards, dones, rows=False):
        """``rows=True``: the large-shape form of the same loop (a test checks that both agree)."""
        r = np.asarray(rewards, dtype=np.float32)
        d = np.asarray(dones)
        T, N = r.shape
        assert N == self.N and d.shape == r.shape
        K = self.K
        new_ret, new_len = [], []
        for t in range(T):
            if rows:   # the same adds, a row of envs at a time (element-wise fp32); the dones still in env order
                self.cur_ret = (self.cur_ret + r[t]).astype(np.float32)
                self.cur_len += 1
            for n in (np.flatnonzero(d[t]) if rows else range(N)):   # chronological: step first, then env index
                if not rows:
                    self.cur_ret[n] = np.float32(self.cur_ret[n] + r[t, n])
                    self.cur_len[n] += 1
                if d[t, n]:
                    self.ring_ret[self.total % K] = self.cur_ret[n]
                    self.ring_len[self.total % K] = self.cur_len[n]
                    self.total += 1
                    new_ret.append(self.cur_ret[n])
                    new_len.append(self.cur_len[n])
                    self.cur_ret[n] = np.float32(0)
                    self.cur_len[n] = 0
        filled = min(self.total, K)
        s = dict.fromkeys(SUMMARY, 0.0)
        s["filled"], s["total"], s["new"] = filled, self.total, len(new_ret)
        if filled:
            x = self.ring_ret[:filled].astype(np.float64)
            mean = x.sum() / filled
            s["ret_mean"] = float(mean)
            s["ret_std"] = float(np.sqrt(((x - mean) ** 2).sum() / filled))
            s["ret_min"], s["ret_max"] = float(x.min()), float(x.max())
            s["len_mean"] = float(self.ring_len[:filled].astype(np.float64).sum() / filled)
        if new_ret:
            s["new_ret_mean"] = float(np.asarray(new_ret, dtype=np.float64).sum() / len(new_ret))
            s["new_len_mean"] = float(np.asarray(new_len, dtype=np.float64).sum() / len(new_len))
        self.summary = s
        return s

    def chronological(self):
        """The window oldest first: (returns, lengths)."""
        K = self.K
        order = [(self.total + i) % K for i in range(K)] if self.total > K else list(range(min(self.total, K)))
        return self.ring_ret[order].copy(), self.ring_len[order].copy()
