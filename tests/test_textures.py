"""The procedural textures' plain-Python restatement (tests/golden/make_kats.py, written from the Java's
myTextureHandler / noise_3d / setTexture) against the oracle, in breadth, on the CPU.

The scenes are the tile scenes of tests/tex_util.py restricted to the tiles the restatement loads (identity
or translated spheres), rendered by the oracle at W x W, 1 spp. Per material a seeded sample of PER_TILE
pixels whose camera ray hits that material's tile is re-derived by the restatement's pixel(row, col, seed)
and held to test_kats.TOL on the float32 frame and to the equal ARGB int.

test_a_deviation_is_caught is the sensitivity proof: one misreading of the Java at a time is patched into
the loaded restatement, and the same comparison must then fail -- some sampled pixel of an affected
material moves by more than 10 x TOL. It decides nothing about the product; it shows that the scenes'
parameters let the comparison tell the Java's reading from its nearest misreadings.

  lowerKey read as floorKey  cannot show on a random scene: the two differ only when a cell's first
  nextDouble EQUALS a key of the pdf table. The `pdf edge` tile of gen_tex_stone has an avgNumPerCell
  searched for exactly that (tex_util.pdf_edge_avg): the cell under the sphere's front point draws the key
  of 2 points, so lowerKey gives it 1 point and floorKey 2.

The conditions that keep the GPU comparison (tests/test_gpu_textures.py) from passing on nothing are decided
on the oracle's output alone, so they are checked here on the full scenes: tex_util.check_conditions."""
import numpy as np
import pytest

from tests import tex_util as tx
from tests import trace_util as tu
from tests.test_kats import TOL

W = 128
PER_TILE = 12
SEED = 0x5EED0001


class Frame:
    """One identity-tile scene: the oracle's frame, each tile's pixels, the restatement's scene."""

    def __init__(self, gen, d):
        c = tx.OracleCase(gen, d, only="identity")
        self.sc = c.sc
        self.text = c.sc.text
        self.rgb, self.argb, _ = c.o.render(W, W, spp=1, seed=SEED)
        o, dd = tu.camera_rays(W, W, c.sc.fov)
        rec = c.o.trace(o, dd, seed=SEED)
        on = c.sc.on_tile(rec["pos"], rec["hit"]).reshape(W, W)
        g = np.random.default_rng(tx.SEED)
        self.sample = {}
        for t in c.sc.tiles:
            px = np.argwhere(on == t.index)
            assert len(px) >= PER_TILE, (t.name, len(px))
            self.sample[t.index] = px[g.choice(len(px), PER_TILE, replace=False)]
        c.close()

    def restated(self, m):
        return m.load(self.text, W, W, textures={k: v.tolist() for k, v in self.sc.textures.items()})

    def worst(self, m, tiles):
        """{tile name: (max |restatement - oracle| over its sampled pixels, ARGB mismatches)}"""
        sc = self.restated(m)
        out = {}
        for t in tiles:
            d, bad = 0.0, 0
            for r, c in self.sample[t.index]:
                got = sc.pixel(int(r), int(c), SEED)
                diff = np.abs(np.asarray(got) - self.rgb[r, c].astype(np.float64))
                d = max(d, float(np.nan_to_num(diff, nan=np.inf).max()))
                bad += int(m.argb(got) != int(self.argb[r, c]))
            out[t.name] = (d, bad)
        return out


@pytest.fixture(scope="module")
def frame_of(tmp_path_factory):
    d = tmp_path_factory.mktemp("tex_frames")
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Frame(tx.GENERATORS[name], d)
        return cache[name]
    return get


@pytest.mark.parametrize("name", ["gen_tex_perlin", "gen_tex_stone", "gen_tex_image"])
def test_restatement_matches_the_oracle(name, frame_of):
    f = frame_of(name)
    tiles = [t for t in f.sc.tiles if not t.facts.get("nan")]
    res = f.worst(tu.make_kats(), tiles)
    print(name, len(tiles), "materials x", PER_TILE, "pixels; worst |d|", max(v[0] for v in res.values()))
    bad = {k: v for k, v in res.items() if not v[0] <= TOL or v[1]}
    assert not bad, bad
    kinds = {t.kind for t in tiles}
    assert kinds >= ({"noise", "marble", "wood", "wood2"} if name == "gen_tex_perlin" else {"stone"} if name == "gen_tex_stone" else {"image"})


def _floor_key(keys, x):
    best = None
    for k in keys:
        if k <= x and (best is None or k > best):
            best = k
    return best


# (what, how the restatement is bent, the scene, the tiles it must show on)
DEVIATIONS = [
    ("last octave dropped", lambda mp, m: mp.setattr(m, "turb_val", lambda p, n, a, f=m.turb_val: f(p, n - 1, a)),
     "gen_tex_perlin", lambda t: t.kind in ("marble", "wood2")),
    ("1.92 read as 2.0", lambda mp, m: mp.setattr(m, "FREQ_STEP", 2.0), "gen_tex_perlin", lambda t: t.kind in ("marble", "wood2")),
    ("clr_ara's noise calls un-permuted", lambda mp, m: mp.setattr(m, "CLR_NOISE_ARGS", ((0, 1, 2),) * 3),
     "gen_tex_perlin", lambda t: t.kind in ("marble", "wood", "wood2")),
    ("Manhattan and Euclid swapped", lambda mp, m: mp.setattr(m, "DIST_FUNCS", {0: m.dist, 1: m.l1_dist}),
     "gen_tex_stone", lambda t: t.kind == "stone"),
    ("lowerKey read as floorKey", lambda mp, m: mp.setattr(m, "lower_key", _floor_key), "gen_tex_stone",
     lambda t: t.facts.get("pdf_edge")),
    ("fastfloor without the negative branch", lambda mp, m: mp.setattr(m, "fastfloor", lambda x: int(x)),
     "gen_tex_stone", lambda t: t.kind == "stone"),
    ("fixDist applied to ROI 6", lambda mp, m: mp.setattr(m, "ROI_FUNCS", {**m.ROI_FUNCS, 6: (m.ROI_FUNCS[6][0], False, True)}),
     "gen_tex_stone", lambda t: t.facts.get("roi") == 6),
    ("brick pair from the hit's own cell", lambda mp, m: mp.setattr(m, "brick_cell", lambda hit, near: hit),
     "gen_tex_stone", lambda t: t.kind == "stone"),
    ("wood colours from the scaled point", lambda mp, m: mp.setattr(m, "wood_color_point", lambda h, scaled: scaled),
     "gen_tex_perlin", lambda t: t.kind == "wood"),
]


@pytest.mark.parametrize("what,bend,scene,affected", DEVIATIONS, ids=[d[0] for d in DEVIATIONS])
def test_a_deviation_is_caught(what, bend, scene, affected, frame_of, monkeypatch):
    f = frame_of(scene)
    m = tu.make_kats()
    tiles = [t for t in f.sc.tiles if affected(t)][:24]
    assert tiles
    bend(monkeypatch, m)
    res = f.worst(m, tiles)
    moved = {k: v[0] for k, v in res.items() if v[0] > 10 * TOL}
    print(what, "moves", len(moved), "of", len(tiles), "materials; largest", max(v[0] for v in res.values()))
    assert moved, (what, res)


def test_fastfloor_deviation_shows_in_the_noise_too(frame_of, monkeypatch):
    """z is negative on every tile, so float noise without fastfloor's negative branch moves every material."""
    f = frame_of("gen_tex_perlin")
    m = tu.make_kats()
    tiles = [t for t in f.sc.tiles if t.kind in ("noise", "marble")][:6]
    monkeypatch.setattr(m, "fastfloor", lambda x: int(x))
    res = f.worst(m, tiles)
    assert all(v[0] > 10 * TOL for v in res.values()), res


@pytest.mark.parametrize("name", list(tx.GENERATORS))
def test_conditions_hold_on_the_oracle(name, tmp_path):
    """Every tile hit by >= 48 of its rays, >= 20 distinct colours per textured tile, mortar and brick on each
    stone tile with a threshold in (0, 1], two brick pairs, useFwdTrans changing the transformed tiles only,
    scaled coordinates beyond 256, planar (u, v) outside [0, 1], the spheres' poles and seam."""
    c = tx.OracleCase(tx.GENERATORS[name], tmp_path)
    fig = tx.check_conditions(c)
    print(name, len(c.sc.tiles), "tiles", len(c.origin), "rays", fig)
    assert 60 <= len(c.origin) // len(c.sc.tiles) <= 128
    c.close()


def test_noise_color_before_the_command_is_forgotten(tmp_path):
    """setTexture starts with resetDfltTxtrVals (myScene.java:714): a noise_color list given before the
    texture command is dropped, one given after it replaces the kind's own colours."""
    m = tu.make_kats()
    for kind in ("marble", "wood", "wood2", "stone"):
        ts = m.TextureState()
        ts.add_color("noise_color 1 0 0".split())
        ts.set_texture([kind])
        own = [list(c) for c in ts.colors]
        assert [1.0, 0.0, 0.0] not in own and len(own) == (10 if kind == "stone" else 2)
        ts.add_color("noise_color named clr_RED".split())
        assert ts.colors == [[1.0, 0.0, 0.0]]
