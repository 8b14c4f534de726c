"""Host-side argument checks and small conversions that the toolbox modules share (neighbors, counts, gpr, ot, autocorr,
image, register, pca, and the toolbox wrappers of ops).  Plain functions: every refusal is a ``ValueError`` that begins
with the caller's ``what``, made before any device work."""
import torch


def ops():
    """the process's ops backend, looked up at the call (tests replace a module's ``_ops``)"""
    from . import engine as E

    return E.ops()


def describe(t):
    """dtype and shape of a tensor, the type's name of anything else: how a refusal names what it got"""
    return f"{t.dtype} {tuple(t.shape)}" if torch.is_tensor(t) else type(t).__name__


def on_device(what, kernels, **tensors):
    """every tensor (None: absent) on one HIP device; ``kernels`` names the caller's kernels in the refusal"""
    devs = {name: t.device for name, t in tensors.items() if t is not None}
    for name, d in devs.items():
        if d.type != "cuda":
            raise ValueError(f"{what}: {name} is on device {str(d)!r}; the {kernels} kernels run on the GPU only and there "
                             "is no host path - move the tensors to the device first")
    if len(set(devs.values())) > 1:
        raise ValueError(f"{what}: the tensors are on different devices: " + ", ".join(f"{n} on {d}" for n, d in devs.items()))


def coords(t, name, what, max_d, D=None, own_max_message=False):
    """coordinates: a floating-point [n >= 1, D] with 1 <= D <= max_d (``own_max_message``: D > max_d is refused in words
    of its own); ``D``: exactly that many"""
    if not torch.is_tensor(t) or t.dim() != 2 or not t.is_floating_point() or t.shape[0] < 1 or t.shape[1] < 1 \
            or (t.shape[1] > max_d and not own_max_message):
        raise ValueError(f"{what}: {name} has shape {describe(t)}; a floating-point [n >= 1, D] with 1 <= D <= {max_d} is needed")
    if t.shape[1] > max_d:
        raise ValueError(f"{what}: {name} has D = {t.shape[1]} coordinates; at most {max_d} are supported")
    if D is not None and t.shape[1] != D:
        raise ValueError(f"{what}: {name} has shape {tuple(t.shape)}; D = {D} coordinates are needed")
    return t


def values(t, name, what, rows):
    """outputs at ``rows`` points: a floating-point [rows, P >= 1]"""
    if not torch.is_tensor(t) or t.dim() != 2 or not t.is_floating_point() or t.shape[0] != rows or t.shape[1] < 1:
        raise ValueError(f"{what}: {name} has shape {describe(t)}; a floating-point [{rows}, P >= 1] is needed")
    return t


def as_device(t, dtype):
    """what a kernel reads: detached, of ``dtype``, contiguous (the tensor itself where it already is)"""
    return t.detach().to(dtype).contiguous()


def chunk_rows(rows_per_chunk, what):
    """rows per launch: None (the caller's default) or a positive whole number, which 3.0 and a numpy integer are"""
    if rows_per_chunk is None:
        return None
    if isinstance(rows_per_chunk, bool) or int(rows_per_chunk) != rows_per_chunk or rows_per_chunk < 1:
        raise ValueError(f"{what}: rows_per_chunk must be a positive integer, not {rows_per_chunk!r}")
    return int(rows_per_chunk)


def view_counts(n_samples_list, N, least_rows=1, least_views=1):
    """-> (the views' row counts through ``int()``, which truncates; whether they are at least ``least_views`` counts of
    at least ``least_rows`` rows each that sum to N).  The caller words the refusal."""
    ns = [int(n) for n in n_samples_list]
    return ns, len(ns) >= least_views and all(n >= least_rows for n in ns) and sum(ns) == N


def view_offsets(ns):
    """the running sum of the views' row counts: V + 1 offsets from 0"""
    off = [0]
    for n in ns:
        off.append(off[-1] + n)
    return off


def require_finite(what, wording, **tensors):
    """no NaN and no infinity in any tensor, with one host read; the first offender in argument order is named by
    ``wording.format(name=, count=)``"""
    counts = [(~torch.isfinite(t)).sum() for t in tensors.values()]
    if len({c.device for c in counts}) > 1:  # (the device check comes after this one in some callers)
        counts = [c.cpu() for c in counts]
    for name, cnt in zip(tensors, torch.stack(counts).tolist()):
        if cnt:
            raise ValueError(f"{what}: " + wording.format(name=name, count=int(cnt)))
