"""Constructed state for the kernels around an accumulation pass (csrc/kernels.hip: ptmi_adapt, ptmi_resolve_counts;
csrc/denoise_variance.hip: ptmi_pass_moments, ptmi_variance_moments) and for the launch order by cost (ptmi_cost_histogram,
ptmi_cost_offsets, ptmi_cost_scatter), given to a context through ptmi_debug_accum_step and ptmi_debug_order_by_cost.

A LAUNCH is a dict of what one ptmi_debug_accum_step takes, everything BY SLOT: sums (n, 3), prev (n, 4: S_{k-1}.xyz, mean),
m2 (n), passes (n; the passes BEFORE the step), queue (slots, or None with n_queue for 0 .. n_queue - 1), params (a dict of
ptmi_adaptive_params' fields, or None), first, spp - plus labels: name -> list of slots.  restate(launch) is the one-step numpy
float32 restatement of THE STOPPING RULE of include/ptmi.h and of the resolve at per-pixel counts; everything expected comes from
it.  tests/test_accum_edge_sets_host.py proves on the restatement alone that each label sits on the edge it names;
tests/test_gpu_accum_edges.py compares the kernels with it, bit for bit.

  tie_launch            M2 == a * a * (float)(k * (k - 1)), its nextafter up and down, delta == 0 so that M2 is the injected one
  pass_count_launch     k = min_passes - 1, min_passes, max_passes (M2 NaN, Inf); k = 50000 and 65536: k * (k - 1) above 2^31
  beyond_launch         k = 65536 with the comparison reached (max_passes 65537: outside ptmi_accum_pass's range, the hook takes it)
  first_launch          first = 1 with a queue: prev, m2, passes of the queued slots are stale and ignored
  nonfinite_launch      NaN, +Inf, -Inf sums, an Inf prev, NaN / negative M2, S == prev, -0 sums; threshold_zero_launch
  progressive_launch    params None
  compaction_launch     queue lengths x survivor patterns x (identity, scattered) queues
  resolve_launch        passes 0, 1, several next to each other, slots left out of the queue
  variance_launch       passes 0 / 1 / 2 side by side, NaN and negative M2, zero and negative luminance (for source = 0)
and slot_pixels (slot -> local pixel for both slot orders), check_compaction, and the cost sets with check_order.
"""
import numpy as np

F = np.float32
U = np.uint32
INF = F(np.inf)
NAN = F(np.nan)
DENORM_MIN = F(1.401298464324817e-45)


def up(x, n=1):
    x = F(x)
    for _ in range(n):
        x = np.nextafter(x, INF)
    return x


def dn(x, n=1):
    x = F(x)
    for _ in range(n):
        x = np.nextafter(x, -INF)
    return x


def bits(a):
    return np.ascontiguousarray(a, F).view(U)


def same(a, b):
    """bit for bit, a NaN equal to a NaN whatever its payload"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


# ------------------------------------------------------------------------------------------------
# slot <-> local pixel, restated from include/ptmi.h (ptmi_debug_accum_step)
# ------------------------------------------------------------------------------------------------
def slot_pixels(width, rows, tile8):
    """(local row, column) of the slots 0 .. width * rows - 1"""
    s = np.arange(width * rows)
    if not tile8:
        return s // width, s % width
    assert width % 8 == 0 and rows % 8 == 0
    tile, i = s >> 6, s & 63
    per_row = width >> 3
    return (tile // per_row) * 8 + (i >> 3), (tile % per_row) * 8 + (i & 7)


def to_pixels(by_slot, width, rows, tile8):
    """a by-slot array (n, ...) as the local row-major image (rows, width, ...)"""
    by_slot = np.asarray(by_slot)
    lr, x = slot_pixels(width, rows, tile8)
    out = np.zeros((rows, width) + by_slot.shape[1:], by_slot.dtype)
    out[lr, x] = by_slot
    return out


def to_slots(image, tile8):
    """the inverse of to_pixels"""
    image = np.asarray(image)
    lr, x = slot_pixels(image.shape[1], image.shape[0], tile8)
    return np.ascontiguousarray(image[lr, x])


# ------------------------------------------------------------------------------------------------
# the restatement: one stopping test (include/ptmi.h, THE STOPPING RULE) and the resolve at counts
# ------------------------------------------------------------------------------------------------
def luminance_step(S, prev_xyz, spp):
    d = (S - prev_xyz).astype(F)
    return ((F(0.2126) * d[:, 0] + F(0.7152) * d[:, 1] + F(0.0722) * d[:, 2]) * (F(1) / F(spp))).astype(F)


def kk_float(k):
    """(float)(k * (k - 1)) with the product in uint32"""
    k = np.asarray(k, U)
    return (k * (k - U(1))).astype(F)


def queue_of(launch):
    return np.arange(launch["n_queue"], dtype=np.int32) if launch["queue"] is None else np.asarray(launch["queue"], np.int32)


def restate(launch):
    """by slot: prev (n, 4), m2, passes after the step; queued, more (the slot goes on), stop; bound (a * a * (float)(k (k - 1)))
    and k of the queued slots; counts; radiance (n, 3).  Slots outside the queue keep their state and are resolved all the same."""
    S = np.asarray(launch["sums"], F); prev = np.asarray(launch["prev"], F).copy()
    m2 = np.asarray(launch["m2"], F).copy(); passes = np.asarray(launch["passes"], U).copy()
    n = len(S)
    q = queue_of(launch)
    assert len(set(q.tolist())) == len(q) and (q >= 0).all() and (q < n).all()
    queued = np.zeros(n, bool); queued[q] = True
    prm = launch["params"]
    with np.errstate(all="ignore"):
        p = np.zeros_like(prev) if launch["first"] else prev
        M2 = np.zeros_like(m2) if launch["first"] else m2
        k = (np.zeros_like(passes) if launch["first"] else passes) + U(1)
        y = luminance_step(S, p[:, :3], launch["spp"])
        delta = y - p[:, 3]
        mean = p[:, 3] + delta / k.astype(F)
        M2n = M2 + delta * (y - mean)
        if prm is None:
            stop = np.zeros(n, bool); bound = np.full(n, NAN)
        else:
            a = F(prm["threshold"]) * (mean + F(prm["floor"]))
            bound = a * a * kk_float(k)
            ki = k.astype(np.int64)
            stop = (ki >= prm["max_passes"]) | ((ki >= prm["min_passes"]) & (M2n <= bound))
        new_prev = prev.copy(); new_prev[queued, :3] = S[queued]; new_prev[queued, 3] = mean[queued]
        new_m2 = np.where(queued, M2n, m2).astype(F)
        new_passes = np.where(queued, k, passes).astype(U)
        counts = (new_passes * U(launch["spp"])).astype(U)
        radiance = (S * (F(1) / counts.astype(F))[:, None]).astype(F)
    return dict(prev=new_prev, m2=new_m2, passes=new_passes, queued=queued, more=queued & ~stop, stop=queued & stop, bound=bound.astype(F),
                k=k, y=y, counts=counts, radiance=radiance)


# ------------------------------------------------------------------------------------------------
# building blocks
# ------------------------------------------------------------------------------------------------
PARAMS = dict(min_passes=4, max_passes=64, threshold=0.05, floor=0.01)


def background(n, seed, k_max=9):
    """n finite slots in the middle of an accumulation: some stop, some go on"""
    rng = np.random.default_rng(seed)
    prev = np.zeros((n, 4), F)
    prev[:, :3] = rng.uniform(0.0, 8.0, (n, 3)); prev[:, 3] = rng.uniform(0.05, 1.5, n)
    sums = (prev[:, :3] + rng.uniform(0.0, 1.5, (n, 3)).astype(F)).astype(F)
    m2 = (rng.uniform(0.0, 1.0, n) ** 6 * 0.5).astype(F)
    passes = rng.integers(1, k_max, n).astype(U)
    return sums, prev, m2, passes


def scattered_queue(n, length, seed):
    """`length` distinct slots of n in no order"""
    return np.random.default_rng(seed).permutation(n)[:length].astype(np.int32)


def make(n, seed, spp=1, params=PARAMS, first=False, queue=None, n_queue=None):
    sums, prev, m2, passes = background(n, seed)
    if queue is not None:
        n_queue = len(queue)
    elif n_queue is None:
        n_queue = n
    return dict(sums=sums, prev=prev, m2=m2, passes=passes, queue=queue, n_queue=n_queue, params=None if params is None else dict(params),
                first=first, spp=spp, labels={})


def put(launch, label, slot, sums=None, prev=None, m2=None, passes=None):
    launch["labels"].setdefault(label, []).append(int(slot))
    if sums is not None: launch["sums"][slot] = sums
    if prev is not None: launch["prev"][slot] = prev
    if m2 is not None: launch["m2"][slot] = m2
    if passes is not None: launch["passes"][slot] = passes


def steady(launch, slot, k):
    """makes slot a pixel at pass k whose pass mean equals its running mean: delta == 0, so mean = y and M2 stays the injected one.
    Returns (y, the bound a * a * (float)(k (k - 1)))"""
    S = launch["sums"][slot:slot + 1]; pxyz = launch["prev"][slot:slot + 1, :3]
    y = luminance_step(S, pxyz, launch["spp"])[0]
    launch["prev"][slot, 3] = y
    launch["passes"][slot] = k - 1
    prm = launch["params"]
    a = F(prm["threshold"]) * (y + F(prm["floor"]))
    return y, F(a * a * kk_float(k))


def free_slots(launch, count, seed=5):
    """`count` slots of the queue that carry no label yet, spread over the launch"""
    taken = {s for v in launch["labels"].values() for s in v}
    q = [int(s) for s in queue_of(launch) if int(s) not in taken]
    pick = np.random.default_rng(seed).permutation(len(q))[:count]
    assert len(pick) == count
    return [q[i] for i in sorted(pick)]


# ------------------------------------------------------------------------------------------------
# the stopping rule
# ------------------------------------------------------------------------------------------------
TIE_TRIPLES = [(4, 0.05, 0.01), (2, 0.1, 0.01), (7, 0.02, 0.25), (300, 0.5, 1e-3)]       # (k, threshold, floor)


def tie_launch(n, k, threshold, floor, per_label=6):
    L = make(n, 100 + k, params=dict(min_passes=2, max_passes=1000, threshold=threshold, floor=floor))
    slots = free_slots(L, 3 * per_label)
    for j, s in enumerate(slots):
        label = ("tie", "tie_up", "tie_dn")[j % 3]
        _, bound = steady(L, s, k)
        put(L, label, s, m2=bound if label == "tie" else (up(bound) if label == "tie_up" else dn(bound)))
    return L


def pass_count_launch(n):
    """min 4, max 65536, spp 1: one launch mixes k = 3, 4, 50000 and 65536"""
    L = make(n, 7, params=dict(min_passes=4, max_passes=65536, threshold=0.05, floor=0.01))
    s = free_slots(L, 12)
    steady(L, s[0], 3); put(L, "k_min_minus_1", s[0], m2=0.0)                   # M2 = 0 would stop at once, were k >= min_passes
    steady(L, s[1], 4); put(L, "k_min", s[1], m2=0.0)
    for j, (label, v) in enumerate((("k_max_nan", NAN), ("k_max_inf", INF), ("k_max_huge", F(3e38)), ("k_max_zero", F(0)))):
        steady(L, s[2 + j], 65536); put(L, label, s[2 + j], m2=v)                # passes 65535: k * (k - 1) = 0xFFFF0000
    for j, label in enumerate(("k_50000_tie", "k_50000_up", "k_50000_dn")):      # 50000 * 49999 > 2^31: negative as an int32
        _, bound = steady(L, s[6 + j], 50000)
        put(L, label, s[6 + j], m2=(bound, up(bound), dn(bound))[j])
    steady(L, s[9], 65535); put(L, "k_below_max_nan", s[9], m2=NAN)              # k = max_passes - 1 with a NaN M2: goes on
    steady(L, s[10], 2); put(L, "k_2", s[10], m2=0.0)
    steady(L, s[11], 1); put(L, "k_1", s[11], m2=0.0, prev=(0, 0, 0, 0), passes=0)
    return L


def beyond_launch(n):
    """k = 65536 where the comparison is reached: max_passes = 65537, which ptmi_accum_pass rejects and the hook takes as given"""
    L = make(n, 8, params=dict(min_passes=4, max_passes=65537, threshold=0.05, floor=0.01))
    s = free_slots(L, 3)
    for j, label in enumerate(("k_65536_tie", "k_65536_up", "k_65536_dn")):
        _, bound = steady(L, s[j], 65536)
        put(L, label, s[j], m2=(bound, up(bound), dn(bound))[j])
    return L


def first_launch(n):
    """first = 1 and a queue that skips slots: the queued slots' prev, m2 and passes are stale and must not be read"""
    L = make(n, 9, first=True, queue=scattered_queue(n, (2 * n) // 3, 19))
    q = queue_of(L)
    for j, s in enumerate(q):
        L["prev"][s] = (NAN, -INF, F(1e30), F(-7)) if j % 2 else (F(3), F(2), F(1), NAN)
        L["m2"][s] = NAN if j % 3 == 0 else F(-1e20)
        L["passes"][s] = U(0xFFFFFFFF) if j % 5 == 0 else U(40 + j)
        L["labels"].setdefault("stale", []).append(int(s))
    rest = np.setdiff1d(np.arange(n), q)
    L["passes"][rest] = (np.arange(len(rest)) % 4).astype(U)                     # 0 .. 3 passes: what the resolve divides by
    L["labels"]["not_queued"] = [int(s) for s in rest]
    return L


NONFINITE_LABELS = ("sum_nan", "sum_pinf", "sum_ninf", "prev_inf", "prev_inf_sum_inf", "m2_nan", "m2_pinf", "m2_negative", "sum_equals_prev", "sum_negative_zero",
                    "m2_nan_at_max")


def nonfinite_launch(n, with_cases=True):
    """The labelled slots hold non-finite or signed values (with_cases False: the same launch with plain values there)."""
    L = make(n, 11, params=dict(min_passes=2, max_passes=9, threshold=0.05, floor=0.01), queue=scattered_queue(n, (3 * n) // 4, 23))
    s = free_slots(L, len(NONFINITE_LABELS))
    slot = dict(zip(NONFINITE_LABELS, s))
    for label in NONFINITE_LABELS:
        L["passes"][slot[label]] = 3                                                 # k = 4: past min_passes, short of max_passes
        L["labels"][label] = [slot[label]]
    L["passes"][slot["m2_nan_at_max"]] = 8                                           # k = 9 = max_passes
    if not with_cases:
        return L
    L["sums"][slot["sum_nan"], 1] = NAN
    L["sums"][slot["sum_pinf"], 0] = INF
    L["sums"][slot["sum_ninf"], 2] = -INF
    L["prev"][slot["prev_inf"], 0] = INF                                             # d.x = finite - Inf
    L["prev"][slot["prev_inf_sum_inf"], 0] = INF; L["sums"][slot["prev_inf_sum_inf"], 0] = INF      # d.x = Inf - Inf
    L["m2"][slot["m2_nan"]] = NAN
    L["m2"][slot["m2_pinf"]] = INF
    steady(L, slot["m2_negative"], 4); L["m2"][slot["m2_negative"]] = -up(F(0), 3)   # three denormal steps below zero
    L["sums"][slot["sum_equals_prev"]] = L["prev"][slot["sum_equals_prev"], :3]      # y = 0
    L["sums"][slot["sum_negative_zero"]] = F(-0.0); L["prev"][slot["sum_negative_zero"], :3] = F(-0.0)
    L["m2"][slot["m2_nan_at_max"]] = NAN
    return L


def nonfinite_single(n, label):
    """the plain launch with the one labelled case in it"""
    L, full = nonfinite_launch(n, False), nonfinite_launch(n, True)
    s = full["labels"][label][0]
    for key in ("sums", "prev", "m2", "passes"):
        L[key][s] = full[key][s]
    return L


def threshold_zero_launch(n):
    """threshold = 0: a = 0 x (mean + floor), only M2 <= 0 stops"""
    L = make(n, 12, params=dict(min_passes=2, max_passes=100, threshold=0.0, floor=0.01))
    s = free_slots(L, 4)
    for j, (label, v) in enumerate((("t0_zero", F(0)), ("t0_negative_zero", F(-0.0)), ("t0_negative", -DENORM_MIN), ("t0_positive", DENORM_MIN))):
        steady(L, s[j], 5); put(L, label, s[j], m2=v)
    return L


def progressive_launch(n):
    L = make(n, 13, params=None, queue=scattered_queue(n, (3 * n) // 4, 29))
    L["m2"][queue_of(L)[::2]] = 0.0                                                  # would stop under any rule
    return L


# ------------------------------------------------------------------------------------------------
# the compaction
# ------------------------------------------------------------------------------------------------
QUEUE_LENGTHS = [1, 63, 64, 65, 255, 256, 257, None]                                 # None: the whole frame
PATTERNS = ("none", "all", "every_other", "lane_0", "lane_63", "random_half")


def survivors(pattern, length):
    """the queue positions that go on"""
    i = np.arange(length)
    if pattern == "random_half":
        return np.random.default_rng(length).random(length) < 0.5
    return dict(none=i < 0, all=i >= 0, every_other=i % 2 == 0, lane_0=i % 64 == 0, lane_63=i % 64 == 63)[pattern]


def claimed_count(pattern, length):
    """how many survivors the pattern's name promises (random_half: whatever its mask holds - the host test bounds it)"""
    if pattern == "random_half":
        return int(survivors(pattern, length).sum())
    return dict(none=0, all=length, every_other=(length + 1) // 2, lane_0=(length + 63) // 64, lane_63=length // 64)[pattern]


def compaction_launch(n, length, pattern, scattered):
    length = n if length is None else length
    queue = scattered_queue(n, length, 1000 + length) if scattered else None
    L = make(n, 31, params=dict(min_passes=2, max_passes=64, threshold=0.05, floor=0.01), queue=queue, n_queue=length)
    q = queue_of(L)
    more = survivors(pattern, length)
    for pos, s in enumerate(q):
        steady(L, s, 2 + pos % 5)
        L["m2"][s] = F(1e30) if more[pos] else F(0)                                  # far above the bound / at most the bound
    L["labels"] = dict(more=[int(s) for s in q[more]], stop=[int(s) for s in q[~more]])
    return L


def check_compaction(queue_in, more_by_position, out):
    """the contract of the next pass's queue (include/ptmi.h: ptmi_debug_accum_step) and nothing stronger"""
    queue_in = np.asarray(queue_in); more = np.asarray(more_by_position, bool); out = [int(v) for v in out]
    want = [int(v) for v in queue_in[more]]
    assert len(out) == len(want), (len(out), len(want))
    assert len(set(out)) == len(out), "a slot is queued twice"
    assert set(out) == set(want), sorted(set(out) ^ set(want))[:8]
    where = {v: i for i, v in enumerate(out)}
    for w0 in range(0, len(queue_in), 64):                                           # one wave: 64 consecutive queue positions
        sw = [int(v) for v in queue_in[w0:w0 + 64][more[w0:w0 + 64]]]
        if sw:
            at = where[sw[0]]
            assert out[at:at + len(sw)] == sw, f"the survivors of positions {w0} .. {w0 + 63} are not contiguous in input order"


# ------------------------------------------------------------------------------------------------
# the resolve at counts, and the state ptmi_denoise_variance (source = 0) reads
# ------------------------------------------------------------------------------------------------
def resolve_launch(n, spp):
    """passes 0 (injected, outside the queue), 1 and several side by side; half of the slots are not queued"""
    L = make(n, 41 + spp, spp=spp, params=dict(min_passes=2, max_passes=12, threshold=0.05, floor=0.01), queue=scattered_queue(n, n // 2, 43))
    L["passes"] = (np.arange(n) % 7).astype(U); L["passes"][np.arange(n) % 7 == 6] = 10
    q = queue_of(L)
    rest = np.setdiff1d(np.arange(n), q)
    L["labels"] = dict(not_queued=[int(s) for s in rest], passes_0=[int(s) for s in rest if L["passes"][s] == 0],
                       passes_1=[int(s) for s in rest if L["passes"][s] == 1])
    return L


VARIANCE_LABELS = ("m2_nan", "m2_negative", "luminance_zero", "luminance_negative", "passes_0", "passes_1", "passes_2")


def variance_launch(width, rows):
    """By PIXEL (local row-major, for a context without slot tiles): nothing is queued - the state is what the filter reads.
    Columns cycle through 0, 1 and 2 passes, so every k < 2 pixel has a k >= 2 neighbour."""
    n = width * rows
    L = make(n, 51, spp=2, params=None, queue=np.zeros(0, np.int32))
    L["passes"] = ((np.arange(n) % width) % 3).astype(U)
    L["passes"][(np.arange(n) // width) % 4 == 3] = 5
    ok = [int(s) for s in np.flatnonzero(L["passes"] >= 2)]
    pick = [ok[(len(ok) * j) // 5 + 1] for j in range(4)]
    put(L, "m2_nan", pick[0], m2=NAN)
    put(L, "m2_negative", pick[1], m2=F(-1e-3))
    put(L, "luminance_zero", pick[2], sums=(0, 0, 0))
    put(L, "luminance_negative", pick[3], sums=(-1.0, -0.5, 0.25))
    for k in range(3):
        L["labels"][f"passes_{k}"] = [int(s) for s in np.flatnonzero(L["passes"] == k)]
    return L


# ------------------------------------------------------------------------------------------------
# the launch order by cost, restated with Python integers
# ------------------------------------------------------------------------------------------------
def order_shift(classes):
    s = 0
    while (256 >> s) > classes and s < 7:
        s += 1
    return s


def cost_class(cost, cost_max, shift):
    return (255 - ((min(int(cost), int(cost_max)) << 8) // (int(cost_max) + 1))) >> shift


def class_steps(cost_max):
    """the costs at which floor(256 c / (cost_max + 1)) steps, and their neighbours"""
    out = set()
    for j in range(257):
        c = -((-j * (cost_max + 1)) // 256)                                          # the smallest cost with floor(...) >= j
        out.update(v for v in (c - 1, c, c + 1) if 0 <= v <= 0xFFFFFFFF)
    return sorted(out)


ORDER_CLASSES = [1, 2, 16, 32, 256, 300]
ORDER_LENGTHS = [1, 255, 256, 257, 1000]


def order_case(label, cost, cost_max, n=None, scattered=False):
    """a cost table and a queue over it: identity (0 .. n - 1), or n scattered entries of the table"""
    cost = np.asarray([int(c) for c in cost], np.uint64).astype(U)
    n = len(cost) if n is None else n
    queue = np.random.default_rng(len(cost) + n).permutation(len(cost))[:n].astype(np.int32) if scattered else None
    return dict(label=label, cost=cost, cost_max=int(cost_max), n=n, queue=queue)


def order_cases():
    rng = np.random.default_rng(77)
    cases = []
    for n in ORDER_LENGTHS:
        for scattered in (False, True):
            cases.append(order_case(f"random_{n}_{'scattered' if scattered else 'identity'}", rng.integers(0, 401, n + (300 if scattered else 0)), 400, n, scattered))
    cases.append(order_case("cost_max_zero", rng.integers(0, 5, 600), 0))                       # everything in the last class, clamped or not
    cases.append(order_case("at_and_above_cost_max", [0, 99, 100, 101, 1000, 0xFFFFFFFF, 50, 100] * 40, 100))
    cases.append(order_case("cost_max_all_ones", [1 << 24, 1 << 31, 0xFFFFFFFF, 0, (1 << 24) - 1, (1 << 24) + 1, (1 << 31) - 1, (1 << 31) + 1] * 50, 0xFFFFFFFF))
    cases.append(order_case("steps_small", class_steps(9) * 30, 9))
    cases.append(order_case("steps_large", class_steps(1000003), 1000003))
    cases.append(order_case("steps_all_ones", class_steps(0xFFFFFFFF), 0xFFFFFFFF, scattered=True))
    return cases


def restate_order(case, classes):
    """(class of every queue position, the histogram, the ends of the classes)"""
    shift = order_shift(classes)
    q = np.arange(case["n"]) if case["queue"] is None else case["queue"]
    cls = np.array([cost_class(case["cost"][e], case["cost_max"], shift) for e in q], np.int64)
    hist = np.bincount(cls, minlength=256)
    return cls, hist, np.cumsum(hist)


def check_order(case, classes, out, hist):
    """the contract of ptmi_debug_order_by_cost and nothing stronger"""
    q = np.arange(case["n"]) if case["queue"] is None else case["queue"]
    cls, want_hist, ends = restate_order(case, classes)
    out = [int(v) for v in out]
    assert len(out) == len(q) and sorted(out) == sorted(int(v) for v in q), "not a permutation of the input queue"
    class_of = {int(e): int(c) for e, c in zip(q, cls)}
    along = [class_of[e] for e in out]
    assert all(a <= b for a, b in zip(along, along[1:])), "classes do not ascend along the ordered queue"
    assert np.array_equal(np.asarray(hist[:256], np.int64), want_hist), "histogram"
    assert np.array_equal(np.asarray(hist[256:], np.int64), ends), "hist[256 + c] is not the end of class c"
    where = {e: i for i, e in enumerate(out)}
    for b0 in range(0, len(q), 256):                                                 # one workgroup of the scatter: 256 consecutive entries
        for c in np.unique(cls[b0:b0 + 256]):
            run = [int(e) for e in q[b0:b0 + 256][cls[b0:b0 + 256] == c]]
            at = where[run[0]]
            assert out[at:at + len(run)] == run, f"class {c}: the entries of block {b0 // 256} are not contiguous in input order"
