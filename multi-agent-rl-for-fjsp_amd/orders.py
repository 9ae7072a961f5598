"""Order books the caller writes, in the layout fjsp_put_orders reads (include/fjsp.h).

A book is one env's list of orders, an order (products, type, colour): products 1..9, type
1..3 (ProductType SMALL / MEDIUM / BIG), colour 1..3 (PackagingColor RED / BLUE / GREEN).  The
device table is int32 [K, N] (env fastest), word = products | type << 4 | colour << 6 — the low
byte of fjsp_env_view.orders — with counts int32 [N] the rows each env uses.  Needs no GPU.
"""
import numpy as np

MAX_ORDERS = 64   # FJSP_MAX_ORDERS: the closed form's order table (the reference has no limit)


def order_word(n, ptype, colour):
    """The table word of one order; ValueError on a field outside its range."""
    n, ptype, colour = int(n), int(ptype), int(colour)
    if not 1 <= n <= 9:
        raise ValueError(f"an order has 1..9 products, got {n}")
    if not 1 <= ptype <= 3:
        raise ValueError(f"product type must be 1..3, got {ptype}")
    if not 1 <= colour <= 3:
        raise ValueError(f"packaging colour must be 1..3, got {colour}")
    return n | (ptype << 4) | (colour << 6)


def encode(books):
    """A list (one entry per env) of lists of (products, type, colour) -> (words int32 [K, N],
    counts int32 [N]), K the longest book; rows past an env's count are 0."""
    books = [list(b) for b in books]
    counts = np.array([len(b) for b in books], np.int32)
    K = int(counts.max()) if len(books) else 0
    if K > MAX_ORDERS:
        raise ValueError(f"a book holds at most {MAX_ORDERS} orders (FJSP_MAX_ORDERS), got {K}")
    words = np.zeros((K, len(books)), np.int32)
    for e, b in enumerate(books):
        for k, o in enumerate(b):
            if len(o) != 3:
                raise ValueError(f"an order is (products, type, colour), got {o!r}")
            words[k, e] = order_word(*o)
    return words, counts


def decode(words, counts=None):
    """The inverse of encode: words [K, N] (anything np.asarray takes), counts [N] (None: K for
    every env) -> a list per env of (products, type, colour) tuples."""
    w = np.asarray(words).astype(np.int64) & 0xFFFFFFFF
    if w.ndim != 2:
        raise ValueError("words must be [K, N]")
    K, N = w.shape
    c = np.full(N, K, np.int64) if counts is None else np.asarray(counts).astype(np.int64).reshape(-1)
    if len(c) != N or (c < 0).any() or (c > K).any():
        raise ValueError("counts must be [N] with every entry in 0..K")
    return [[(int(x & 15), int((x >> 4) & 3), int((x >> 6) & 3)) for x in w[:int(c[e]), e]] for e in range(N)]


def from_env_view(view):
    """The book of an env read back with FJSPVecEnv.read_env (fjsp_env_view): its num_orders orders."""
    return [(int(w) & 15, (int(w) >> 4) & 3, (int(w) >> 6) & 3) for w in list(view.orders)[:int(view.num_orders)]]


__all__ = ["MAX_ORDERS", "order_word", "encode", "decode", "from_env_view"]
