"""The numpy twin of csrc/lidf_select.hip (losses.topk_mean): the mean of the k largest float32 values and the
backward's weights, with the order and the tie rule the kernels are held to.

  order   torch.topk's: NaN greatest, then +inf ... -inf; -0.0 == +0.0; every NaN equals every NaN
  ties    at the k-th value the lowest indices win: the selection is the first k of (value descending, index ascending)
  k       int(count * ratio), a double product (count = n unless given)
  mean    a float64 sum over the selected float32 values, divided by k (NaN for k == 0)
  weights float32(1 / k) at the selected elements, 0 elsewhere
"""
import numpy as np


def order_key(values):
    """uint32 keys (as int64) that ascend with torch.topk's order of the float32 `values`."""
    v = np.ascontiguousarray(values, dtype=np.float32).reshape(-1)
    b = v.view(np.uint32).astype(np.int64)
    b = np.where(b == 0x80000000, 0, b)                       # -0.0 -> +0.0
    key = np.where(b & 0x80000000, 0xffffffff - b, b | 0x80000000)
    return np.where(np.isnan(v), 0xffffffff, key)             # every NaN: the one greatest key


def k_of(count, ratio):
    return int(count * ratio)


def topk_mean_ref(values, ratio, count=None):
    """dict: k, sel (the selected indices, ascending), mean64, weights [n] float32, scale = sum|selected| / k."""
    v = np.ascontiguousarray(values, dtype=np.float32).reshape(-1)
    n = v.shape[0]
    k = k_of(n if count is None else count, ratio)
    assert 0 <= k <= n
    key = order_key(v)
    order = np.lexsort((np.arange(n), -key))
    sel = np.sort(order[:k])
    w = np.zeros(n, dtype=np.float32)
    with np.errstate(all="ignore"):
        picked = v[sel].astype(np.float64)
        mean64 = picked.sum() / k if k else float("nan")
        scale = np.abs(picked).sum() / k if k else float("nan")
    if k:
        w[sel] = np.float32(1.0 / k)
    return {"k": k, "sel": sel, "mean64": float(mean64), "weights": w, "scale": float(scale)}
