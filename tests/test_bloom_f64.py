"""The bloom's numpy float32 restatement (tests/bloom_ref.py, which the GPU equals bit for bit) against the float64 statement of DESIGN.md §12
(tests/bloom_f64.py: dense per-axis operators, G = P b), and what can be read off P: rows, signs, the diagonal and the column sums.  No GPU.

The bound (`bound`).  u = 2^-24; every f32 operation returns its exact result times (1 + d), |d| <= u.  The inputs of `inputs` keep every pixel either
not light by construction (Y is 0, negative, NaN or Inf in both precisions) or with three non-negative channels and Y > 1e-6 (a rendered frame: below), so the validity of a
pixel is the same decision in both precisions (asserted: no pixel is excluded), Y is a sum of non-negative terms, and b >= 0.

  * m = sums / count: 1 operation, |dm_c| <= u |m_c|.
  * Y: three products and two sums of non-negative terms over m: |dY| <= 4u Y.
  * Bright part, w = Yb / Y in [0, 1] (Y - t <= Y; soft <= q / 2 and q <= Y for knee <= 1).  Yb is continuous in Y, so only errors add up:
    max and min of two values move by no more than the larger move of the two; `Y - t` is chosen only for Y >= t, where it moves by
    4u Y + u (Y - t) <= 5u Y.  q = clip((Y - t) + tk, 0, 2 tk) moves by dq <= 4u Y + u t + u tk + 2u tk <= 4u (Y + t) wherever soft can be chosen
    (Y <= t + 2 tk <= 3t), and soft = q q / (4 tk + 1e-5) by 4u soft + dq q / (2 tk) (four roundings: tk, the square, the sum, the quotient).
    For Y >= t: q <= 2 tk <= 2 Y, so dsoft / Y <= 4u + 8u.  For Y < t: q <= knee Y, so dsoft / Y <= 2u + 4u (2t) knee / (2 tk) = 6u.  So
    dYb / Y <= 12u, dw <= u w + dYb / Y + w dY / Y <= 17u, and b_c = m_c w: |db_c| <= (17 + 2) u |m_c|.  K_B = 20 leaves room for the second-order terms.
  * One level down, per axis, h = (0.125 p0 + 0.375 p1) + (0.375 p2 + 0.125 p3): 0.125 p is exact, the two products by 0.375, the two inner sums and
    the outer sum round: at most (0.75 + 1 + 1) u max|p| <= 3u max|p|; the weights sum to 1, so the inputs' errors pass on with weight <= 1.
    6 operations per level, and every value of every level is a convex combination of the b its support sees.
  * One step up, per axis, 0.75 near + 0.25 far: (0.75 + 1) u <= 2u; 4 operations per level.
  * The blend U_l = (1 - s) D_l + s up(U_{l+1}): 1 - s rounds once, both products and the sum round: (2 (1 - s) + s + 1) u <= 3u, on top of the larger of
    its inputs' errors, which is the way through `up` (4 more).  7 operations per blended level on the longest chain.
  * So |dG| <= N_G u Bmax + K_B u Mmax with N_G = 6 L + 7 (L - 1) + 4 = 13 L - 3, Bmax = the largest b_c and Mmax = the largest m_c of a light pixel among
    the inputs that the output's row of P is positive on.
  * The composite m + i (G - b): G, b >= 0, so |G - b| <= Bmax: the difference, the product and the sum round, <= u (2 Bmax + |out|), and
    |out| <= |m_c| + Bmax; dm_c = u |m_c|; i (dG + db) <= dG + K_B u Mmax.

  * A rendered frame can hold a light pixel with a negative channel.  Then Y is no sum of non-negative terms: |dY| <= 4u kappa Y with
    kappa = (0.2126 |m_r| + 0.7152 |m_g| + 0.0722 |m_b|) / Y >= 1, every term of the bright part that came from dY / Y grows by kappa, and Mmax is taken
    over kappa |m_c|; b_c can be negative, so Bmax is taken over |b_c|, |G - b| <= 2 Bmax and the composite's three operations give 6 Bmax, not 3.
    The synthetic inputs have kappa = 1; the bound below is the general one for all of them.

    |out_f32 - out_f64| <= u (1 + 1e-4) ((13 L + 3) Bmax + 2 K_B Mmax + 2 |m_c|) + 64 * 2^-149

L = 6: 81 Bmax + 40 Mmax + 2 |m|.  The factor 1 + 1e-4 covers the products of two errors (at most about 120 u of the first-order terms) and the last term
a subnormal rounding in each of fewer than 64 operations on any chain.  The bound comes from the float64 statement alone.  Largest measured
|out_f32 - out_f64| / bound over every size, input and setting below: just under 0.05; 0.023 on the device."""
import itertools

import numpy as np
import pytest

import bloom_f64 as b64
import bloom_ref as bl

U = 2.0 ** -24
K_B = 20
SIZES = [(16, 8), (48, 40), (80, 56), (208, 120)]
PLANS = {(16, 8): [(8, 4), (4, 2)],
         (48, 40): [(24, 20), (12, 10), (6, 5), (3, 3), (2, 2)],
         (80, 56): [(40, 28), (20, 14), (10, 7), (5, 4), (3, 2)],
         (208, 120): [(104, 60), (52, 30), (26, 15), (13, 8), (7, 4), (4, 2)]}
LEVELS = (1, 2, 6, 10)
THRESHOLDS, KNEES, CLAMPS, SPREADS, INTENSITIES = (0.0, 0.02, 1.0), (0.0, 0.5, 1.0), (0.0, 0.5), (0.0, 0.7, 1.0), (0.0, 0.05, 1.0)

_INPUTS = {}


def impulse_spots(W, H):
    """The four corners, the middle of each edge, one pixel inside each edge, the interior."""
    return [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, 0), (W // 2 - 1, H - 1), (0, H // 2), (W - 1, H // 2 - 1),
            (W // 3, 1), (W // 3 + 1, H - 2), (1, H // 3), (W - 2, H // 3 + 1), (W // 2, H // 2), (W // 3, H // 3), (W // 3 + 1, H // 3)]


def inputs(W, H):
    """name -> (W, H, 3) float32 sums, made once per size.  Light pixels have non-negative channels and a luminance above 1e-6 at every count used."""
    if (W, H) in _INPUTS:
        return _INPUTS[(W, H)]
    rng = np.random.default_rng(1200 * W + H)
    random = (np.exp2(rng.uniform(-9.0, 3.0, (W, H, 1))) * rng.uniform(0.5, 1.5, (W, H, 3))).astype(np.float32)
    impulses = np.zeros((W, H, 3), np.float32)
    for k, (i, j) in enumerate(impulse_spots(W, H)):
        impulses[i, j] = (40.0 + k, 25.0 - k, 10.0 + 3 * k)
    rectangle = np.full((W, H, 3), 0.01, np.float32)
    rectangle[:max(W // 3, 3), :max(H // 2, 3)] = (6.0, 5.0, 3.0)              # touches the left and the top border
    constant = np.full((W, H, 3), 0.4, np.float32)
    dirty = random.copy()
    k = rng.permutation(W * H)[:max(W * H // 20, 8)]
    values = np.array([(0, 0, 0), (-1.0, -2.0, -0.5), (np.nan, 1, 1), (np.inf, 1, 1), (-np.inf, 0, 0), (np.inf, -np.inf, 0), (1, np.nan, np.nan),
                       (np.inf, np.inf, np.inf)], np.float32)
    dirty.reshape(-1, 3)[k] = values[np.arange(len(k)) % len(values)]
    _INPUTS[(W, H)] = dict(random=random, impulses=impulses, rectangle=rectangle, constant=constant, dirty=dirty)
    return _INPUTS[(W, H)]


class Statement:
    """The float64 statement of one (sums, counts, threshold, knee, clamp, levels, spread) with the two scales of the bound; every intensity shares it."""

    def __init__(self, sums, samples, fs, threshold=0.0, knee=0.5, clamp=0.0, bright=None, m_max=None, y_min=1e-6):
        self.fs, self.L = fs, len(fs)
        self.m = b64.mean_of(sums, samples)
        self.b, self.valid, self.Y = bright if bright is not None else b64.bright(self.m, threshold, knee, clamp)
        light = self.valid
        # the one decision, the validity of a pixel, is the same in both precisions by construction: no pixel is excluded
        assert (light | ~(self.Y > 0) | ~np.isfinite(self.Y)).all() and (self.Y[light] > y_min).all()
        self.G = b64.apply(fs, self.b)
        self.b_max = b64.support_max(fs, np.abs(self.b))
        with np.errstate(all="ignore"):
            kappa = np.where(light, b64.luminance(np.abs(self.m)) / self.Y, 0.0)           # 1 where no channel is negative
            scaled = np.where(light[..., None], np.abs(self.m) * kappa[..., None], 0.0)
        self.m_max = m_max if m_max is not None else b64.support_max(fs, scaled)
        self.own = np.where(np.isfinite(self.m), np.abs(self.m), 0.0)

    def out(self, intensity):
        with np.errstate(all="ignore"):
            return self.m + float(np.float32(intensity)) * (self.G - self.b)

    def bound(self):
        """The docstring's bound per pixel and channel."""
        return U * (1 + 1e-4) * ((13 * self.L + 3) * self.b_max + 2 * K_B * self.m_max + 2 * self.own) + 64 * 2.0 ** -149


def compare(got, st, intensity, what):
    """Hold `got` (f32, from the restatement or the device) to the float64 statement; returns the largest ratio to the bound."""
    out64 = st.out(intensity)
    finite = np.isfinite(out64)
    got = np.asarray(got, dtype=np.float64)
    assert (np.isnan(got) == np.isnan(out64)).all(), what
    inf = np.isinf(out64)
    assert (got[inf] == out64[inf]).all(), what                                 # an Inf of its own input stays that Inf
    bd = st.bound()
    ratio = np.abs(got[finite] - out64[finite]) / bd[finite]
    worst = float(ratio.max())
    assert worst <= 1.0, (what, worst)
    return worst


_FACTORS = {}


def factors(W, H, levels, spread):
    L = len(b64.plan(W, H, levels)) - 1
    if (W, H, L, spread) not in _FACTORS:
        _FACTORS[(W, H, L, spread)] = b64.factors(W, H, levels, spread)
    return _FACTORS[(W, H, L, spread)]


# ---------------------------------------------------------------- 1. the level plan, from the sentence
@pytest.mark.parametrize("size", SIZES)
def test_level_plan(size):
    W, H = size
    assert b64.plan(W, H, 10)[1:] == PLANS[size]
    for levels in LEVELS:
        want = PLANS[size][:max(1, min(levels, len(PLANS[size])))]
        assert b64.plan(W, H, levels)[1:] == want
        assert bl.levels_used(W, H, levels) == len(want) and bl.level_sizes(W, H, len(want))[1:] == want
    assert len(b64.plan(1920, 1080, 10)) - 1 == 10 and b64.plan(1920, 1080, 6)[1:] == [(960, 540), (480, 270), (240, 135), (120, 68), (60, 34), (30, 17)]


# ---------------------------------------------------------------- 2. the restatement against the float64 statement
@pytest.mark.parametrize("size", SIZES)
def test_restatement_within_the_derived_bound(size):
    W, H = size
    worst = 0.0
    for name, sums in inputs(W, H).items():
        m_max = {}
        for t, k, c in itertools.product(THRESHOLDS, KNEES, CLAMPS):
            bright = b64.bright(b64.mean_of(sums, 1), t, k, c)
            made = {}                                                  # levels that the plan reduces to the same L share one statement
            for levels, spread in itertools.product(LEVELS, SPREADS):
                fs = factors(W, H, levels, spread)
                if (len(fs), spread) not in made:
                    made[(len(fs), spread)] = Statement(sums, 1, fs, bright=bright, m_max=m_max.get((len(fs), spread)))
                st = made[(len(fs), spread)]
                m_max[(len(fs), spread)] = st.m_max
                for i in INTENSITIES:
                    kw = dict(intensity=i, threshold=t, knee=k, clamp=c, spread=spread, levels=levels)
                    worst = max(worst, compare(bl.bloom(sums, 1, **kw)[0], st, i, (name, kw)))
    print("bloom %dx%d: largest |ref - f64| / bound = %.4f" % (W, H, worst))


def test_the_count_divides_in_both():
    """spp 3 and per-pixel counts: the division is in, and the bound's one operation for it holds."""
    W, H = 48, 40
    counts = np.repeat(np.repeat(np.random.default_rng(5).integers(1, 9, (W // 8, H // 8)) * 4, 8, axis=0), 8, axis=1)
    kw = dict(intensity=0.4, threshold=0.02, knee=0.5, clamp=0.0, spread=0.7, levels=6)
    for name, sums in inputs(W, H).items():
        for samples in (3, counts):
            st = Statement(sums, samples, factors(W, H, 6, 0.7), 0.02, 0.5, 0.0)
            compare(bl.bloom(sums, samples, **kw)[0], st, 0.4, name)


# ---------------------------------------------------------------- 3. what P says
@pytest.mark.parametrize("size", SIZES + [(64, 64), (120, 68)])
def test_rows_signs_and_diagonal_of_P(size):
    W, H = size
    for levels, spread in itertools.product(LEVELS, SPREADS):
        fs = b64.factors(W, H, levels, spread)
        assert abs(sum(c for c, _, _ in fs) - 1.0) < 1e-15 and all(c >= 0 for c, _, _ in fs)
        assert all((ax >= 0).all() and (ay >= 0).all() for _, ax, ay in fs)                  # every entry of P is >= 0
        assert np.abs(b64.row_sums(fs) - 1.0).max() < 1e-13                                  # every row sums to 1: a constant stays constant
        assert b64.diagonal(fs).max() <= 0.25 + 1e-15                                        # no identity part: at most 1/4 of a pixel stays in place
    const = b64.apply(b64.factors(W, H, 6, 0.7), np.full((W, H, 3), 0.4))
    assert np.abs(const - 0.4).max() < 1e-15


def test_dense_P_is_its_factors_and_an_impulse_reads_its_column():
    W, H = 16, 8
    fs = b64.factors(W, H, 6, 0.7)
    P = b64.dense(fs)
    assert np.abs(P.sum(axis=1) - 1).max() < 1e-14 and P.min() >= 0 and P.diagonal().max() < 1
    assert np.abs(P.sum(axis=0).reshape(W, H) - b64.column_sums(fs)).max() < 1e-14
    for i, j in impulse_spots(W, H):
        e = np.zeros((W, H)); e[i, j] = 1.0
        assert np.abs(b64.apply(fs, e).reshape(-1) - P[:, i * H + j]).max() < 1e-15
        G32 = bl.glow(np.repeat(e[..., None], 3, axis=2).astype(np.float32), 0.7, 6)[..., 0]
        assert np.abs(G32 - P[:, i * H + j].reshape(W, H)).max() <= (13 * 2 - 3) * U


# max |column sum - 1| over all inputs at levels = 10, by size and spread, as measured on the float64 operators (4 decimals)
COLUMN_WORST = {(16, 8): {0.7: 0.0, 1.0: 0.0}, (64, 64): {0.7: 0.0, 1.0: 0.0},
                (48, 40): {0.7: 0.1948, 1.0: 0.7578}, (80, 56): {0.7: 0.1822, 1.0: 0.7051},
                (208, 120): {0.7: 0.3557, 1.0: 1.7374}, (120, 68): {0.7: 1.3133, 1.0: 6.0895}}
INTERIOR_WORST = 1.5e-3        # inputs at least 2^(L+1) pixels from every border: 0 everywhere but 120x68 at four levels (1.46e-3 at spread 1, 5.0e-4 at 0.7)


@pytest.mark.parametrize("size", sorted(COLUMN_WORST))
def test_column_sums_energy_is_conserved_only_while_every_halved_level_is_even(size):
    """Row sums 1 keep a constant image constant; conservation of energy is the column sums, every input's total weight over all outputs.  A level down
    gives every input the total weight 1/2 per axis and a level up 2, clamped indices included, as long as the level that is halved has an even size.
    At an odd size n the last output ((n + 1) >> 1 of them) reads 2x+1 and 2x+2 past the end, both clamped onto the last sample, which then weighs 1
    instead of 1/2: light near the far (right, bottom) border is counted up to twice per odd level, and the near border loses a little to the
    renormalisation further up.  So: exact conservation where no halved level is odd; elsewhere the recorded worst case."""
    W, H = size
    for levels in (1, 2, 3, 4, 5, 6, 10):
        sizes = b64.plan(W, H, levels)
        L = len(sizes) - 1
        even = all(w % 2 == 0 and h % 2 == 0 for w, h in sizes[:-1])
        for spread in SPREADS:
            cs = b64.column_sums(b64.factors(W, H, levels, spread))
            off = np.abs(cs - 1.0)
            assert abs(cs.mean() - 1.0) < 1e-13                       # rows sum to 1, so the image's mean weight is 1: gains and losses balance
            if even or spread == 0.0 or L == 1:
                assert off.max() < 1e-13, (levels, spread)            # to rounding, borders included
            else:
                assert off.max() > 0.04, (levels, spread)             # not conserved: more than 4 % at some input
            d = 2 ** (L + 1)
            inner = off[d:W - d, d:H - d]
            if inner.size:
                assert inner.max() <= INTERIOR_WORST, (levels, spread)
                if size != (120, 68) or L != 4:
                    assert inner.max() < 1e-13, (levels, spread)
            if levels == 10 and spread > 0:
                assert abs(off.max() - COLUMN_WORST[size][spread]) < 5e-5, (spread, off.max())
                if COLUMN_WORST[size][spread] > 0:                     # the excess sits on the far border
                    assert np.unravel_index(off.argmax(), off.shape) == (W - 1, H - 1)


def test_the_interior_impulse_test_of_the_restatement_sees_none_of_this():
    """64x64 halves to even sizes throughout: there the restatement's sum is the input's to rounding, at the border too."""
    W = H = 64
    b = np.zeros((W, H, 3), np.float32)
    for i, j in impulse_spots(W, H):
        b[i, j] = 1.0
    for levels in (3, 6):
        G = bl.glow(b, 0.7, levels).astype(np.float64)
        assert abs(G.sum() / b.sum() - 1.0) < 13 * 6 * U
