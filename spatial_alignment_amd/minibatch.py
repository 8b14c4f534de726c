"""Minibatch (stochastic variational) training over per-view row samples.

Given the M x M factors, every row's likelihood term of the sparse variational GP is independent of the others.  A
step may therefore see B_v rows of view v only, their log-likelihood weighted by N_v / B_v, the KL terms whole: the
loss is an unbiased estimate of the full negative ELBO, and its gradient of the full gradient, at the cost of a
B-row problem.

``RowSampler`` draws step t's batch on the device (``torch.ops.gpsa.row_sample_gather``, csrc/minibatch.hip) into
buffers that persist across steps, and advances its step counter there too: nothing is read back by the host, so the
draw can sit inside a captured step (``train.GraphedTrainStep(..., sampler=...)``) and every replay trains on the next
batch.  The batch's ``data_dict`` carries ``view_weights`` = N_v / B_v, which ``loss_fn`` applies through
``gpsa_elbo_loss_weighted_fwd`` / ``_bwd``.  A Poisson modality's ``log_offset`` (per-row log size factors) is gathered
with the rows by a second call of the same op.

The index rule (standard drop-last epochs): K = N div B batches per epoch; step t is slot k = t mod K of epoch
e = t div K, and row j of the batch of (modality m, view v) is  pi_{seed,m,v,e}(k B + j),  pi a keyed bijection of
[0, N) - no sort, no stored permutation; the rows of a batch are distinct and, when B divides N, an epoch's batches
partition the view.  ``feistel_perm`` below is the host restatement of the device's pi, bit for bit.
"""
import numpy as np
import torch

_M64 = (1 << 64) - 1
_GOLDEN = 0x9E3779B97F4A7C15
ROUNDS = 6
MAX_PAIRS = 64  # (modality, view) pairs one sampler covers (gpsa_row_sample_gather)


def _mix64(z):
    """splitmix64's finaliser on a Python int (mod 2^64)"""
    z &= _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def _mix64_np(z):
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def perm_key(seed, m, v, e):
    """base key of pi_{seed, m, v, e}"""
    h = _mix64(int(seed))
    h = _mix64(h ^ int(m))
    h = _mix64(h ^ int(v))
    return _mix64(h ^ int(e))


def feistel_perm(x, N, seed, m, v, e):
    """pi_{seed,m,v,e}(x) for an array of x in [0, N): a 6-round alternating Feistel network on k = ceil(log2 N) bits
    (high half A of k // 2 bits, low half B of the rest; even rounds A ^= F(B), odd rounds B ^= F(A), F = splitmix64
    finaliser of the round key ^ the other half), cycle-walked until the value is below N"""
    N = int(N)
    if N < 1:
        raise ValueError(f"feistel_perm: N = {N}")
    k = max(0, (N - 1).bit_length())
    a = k >> 1
    b = k - a
    ma, mb = np.uint64((1 << a) - 1), np.uint64((1 << b) - 1)
    base = perm_key(seed, m, v, e)
    keys = [np.uint64(_mix64(base ^ (((r + 1) * _GOLDEN) & _M64))) for r in range(ROUNDS)]
    y = np.asarray(x, dtype=np.uint64).copy()
    if y.size and (int(y.max()) >= N):
        raise ValueError("feistel_perm: x outside [0, N)")
    todo = np.ones(y.shape, dtype=bool)
    while todo.any():
        z = y[todo]
        A, B = z >> np.uint64(b), z & mb
        for r in range(ROUNDS):
            if r % 2 == 0:
                A = A ^ (_mix64_np(keys[r] ^ B) & ma)
            else:
                B = B ^ (_mix64_np(keys[r] ^ A) & mb)
        z = (A << np.uint64(b)) | B
        y[todo] = z
        todo[todo] = z >= np.uint64(N)
    return y.astype(np.int64)


def batch_indices(N, B, seed, m, v, t):
    """the view-local rows of step t's batch of (modality m, view v): [B] int64"""
    N, B, t = int(N), int(B), int(t)
    K = N // B
    e, k = divmod(t, K)
    return feistel_perm(np.arange(k * B, k * B + B), N, seed, m, v, e)


def _as_batch_sizes(batch_size, mods, views):
    """int or {mod: [B_v]} -> {mod: [B_v]}"""
    if isinstance(batch_size, dict):
        if set(batch_size) != set(mods):
            raise ValueError(f"RowSampler: batch_size names modalities {sorted(batch_size)}, the model {sorted(mods)}")
        out = {}
        for m in mods:
            bs = list(batch_size[m])
            if len(bs) != len(views[m]):
                raise ValueError(f"RowSampler: {len(bs)} batch sizes for the {len(views[m])} views of {m!r}")
            out[m] = bs
        return out
    return {m: [batch_size] * len(views[m]) for m in mods}


class Batch:
    """one step's batch; the same tensors at every step (plans, the view_rows memo and captured graphs see stable
    pointers): ``data_dict`` ({mod: spatial_coords, outputs, n_samples_list = [B_v], view_weights = N_v / B_v}),
    ``X`` ({mod: coordinates}), ``view_idx`` / ``Ns`` (model.create_view_idx_dict of the batch), ``rows`` ({mod: int64
    row numbers into the full data})"""

    def __init__(self, data_dict, X, view_idx, Ns, rows):
        self.data_dict, self.X, self.view_idx, self.Ns, self.rows = data_dict, X, view_idx, Ns, rows


class RowSampler:
    """Draws per-view row samples of ``data_dict`` for minibatch training of ``model``.

    ``batch_size``: rows per view, an int for every view or ``{mod: [B_v]}``, 1 <= B_v <= N_v.  ``seed``: an int in
    [0, 2^63).  ``next()`` draws the next step's batch on the device and returns the (persistent) ``Batch``."""

    def __init__(self, model, data_dict, batch_size, seed=0):
        mods = list(model.modality_names)
        dev = model.Xtilde.device
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < (1 << 63):
            raise ValueError(f"RowSampler: seed must be an int in [0, 2^63), not {seed!r}")
        if set(data_dict) != set(mods):
            raise ValueError(f"RowSampler: data_dict holds {sorted(data_dict)}, the model {sorted(mods)}")
        views = {}
        for m in mods:
            d = data_dict[m]
            X, Y = d.get("spatial_coords"), d.get("outputs")
            for name, t in (("spatial_coords", X), ("outputs", Y)):
                if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 2:
                    raise ValueError(f"RowSampler: data_dict[{m!r}][{name!r}] must be a 2-D float32 tensor")
            sizes = [int(n) for n in d["n_samples_list"]]
            if len(sizes) != model.n_views:
                raise ValueError(f"RowSampler: modality {m!r} has {len(sizes)} views, the model {model.n_views}")
            if sum(sizes) != X.shape[0] or X.shape[0] != Y.shape[0]:
                raise ValueError(f"RowSampler: n_samples_list of {m!r} sums to {sum(sizes)}, its data holds "
                                 f"{X.shape[0]} / {Y.shape[0]} rows")
            views[m] = sizes
        bs = _as_batch_sizes(batch_size, mods, views)
        for m in mods:
            for v, (n, b) in enumerate(zip(views[m], bs[m])):
                if isinstance(b, bool) or not isinstance(b, (int, np.integer)) or not 1 <= int(b) <= n:
                    raise ValueError(f"RowSampler: batch size {b!r} of view {v} of {m!r} is outside [1, {n}]")
        if sum(len(views[m]) for m in mods) > MAX_PAIRS:
            raise ValueError(f"RowSampler: more than {MAX_PAIRS} (modality, view) pairs")
        if dev.type != "cuda":
            raise ValueError("RowSampler: the model is not on a HIP device (the sampler is a device kernel)")
        for m in mods:
            for name in ("spatial_coords", "outputs"):
                if data_dict[m][name].device != dev:
                    raise ValueError(f"RowSampler: data_dict[{m!r}][{name!r}] is not on the model's device {dev}")
        self.model, self.mods, self.seed = model, mods, int(seed)
        self.views = views
        self.batch_size = {m: [int(b) for b in bs[m]] for m in mods}
        self._X = [data_dict[m]["spatial_coords"].contiguous() for m in mods]
        self._Y = [data_dict[m]["outputs"].contiguous() for m in mods]
        self.counter = torch.zeros(1, dtype=torch.int64, device=dev)
        tot = {m: sum(self.batch_size[m]) for m in mods}
        self._rows = [torch.zeros(tot[m], dtype=torch.int64, device=dev) for m in mods]
        self._Xb = [torch.zeros(tot[m], x.shape[1], dtype=torch.float32, device=dev) for m, x in zip(mods, self._X)]
        self._Yb = [torch.zeros(tot[m], y.shape[1], dtype=torch.float32, device=dev) for m, y in zip(mods, self._Y)]
        # per-row log offsets (count outputs: model.likelihood): gathered as one more "output" column by a second call of
        # the op on a step counter of its own, which moves in lockstep with the first (same seed, same step, same rows)
        self._O = self._Ob = self._counter_o = None
        if any(data_dict[m].get("log_offset") is not None for m in mods):
            self._O, self._Ob = [], []
            for m, x in zip(mods, self._X):
                o = data_dict[m].get("log_offset")
                if o is None:
                    o = torch.zeros(x.shape[0], dtype=torch.float32, device=dev)
                elif (not torch.is_tensor(o) or o.dtype != torch.float32 or tuple(o.shape) != (x.shape[0],)
                      or o.device != dev):
                    raise ValueError(f"RowSampler: data_dict[{m!r}]['log_offset'] must be a float32 tensor of shape "
                                     f"({x.shape[0]},) on {dev}")
                self._O.append(o.contiguous().view(-1, 1))
                self._Ob.append(torch.zeros(tot[m], 1, dtype=torch.float32, device=dev))
            self._counter_o = torch.zeros(1, dtype=torch.int64, device=dev)
            self._rows_o = [torch.zeros_like(r) for r in self._rows]
            self._Xb_o = [torch.zeros_like(x) for x in self._Xb]
        dd = {}
        for i, m in enumerate(mods):
            w = torch.tensor([n / b for n, b in zip(views[m], self.batch_size[m])], dtype=torch.float64, device=dev)
            dd[m] = {"spatial_coords": self._Xb[i], "outputs": self._Yb[i], "n_samples_list": list(self.batch_size[m]),
                     "view_weights": w}
            if self._O is not None and data_dict[m].get("log_offset") is not None:
                dd[m]["log_offset"] = self._Ob[i].view(-1)
        view_idx, Ns, _, _ = model.create_view_idx_dict(dd)
        self.batch = Batch(dd, {m: dd[m]["spatial_coords"] for m in mods}, view_idx, Ns,
                           {m: r for m, r in zip(mods, self._rows)})
        self._args = ([len(views[m]) for m in mods], [n for m in mods for n in views[m]],
                      [b for m in mods for b in self.batch_size[m]])

    def next(self):
        """draw the batch of step ``counter`` into the persistent buffers, advance the counter (device only)"""
        nv, nr, bs = self._args
        torch.ops.gpsa.row_sample_gather(self._X, self._Y, nv, nr, bs, self.seed, self.counter, self._rows, self._Xb,
                                         self._Yb)
        if self._O is not None:
            torch.ops.gpsa.row_sample_gather(self._X, self._O, nv, nr, bs, self.seed, self._counter_o, self._rows_o,
                                             self._Xb_o, self._Ob)
        return self.batch

    def set_step(self, t):
        """the next ``next()`` draws step t's batch"""
        self.counter.fill_(int(t))
        if self._counter_o is not None:
            self._counter_o.fill_(int(t))

    def host_rows(self, t):
        """{mod: int64 rows} of step t's batch from the host restatement (tests, documentation)"""
        out = {}
        for i, m in enumerate(self.mods):
            parts, off = [], 0
            for v, (n, b) in enumerate(zip(self.views[m], self.batch_size[m])):
                parts.append(off + batch_indices(n, b, self.seed, i, v, t))
                off += n
            out[m] = np.concatenate(parts)
        return out
