"""The case table of tests/test_gpu_large_batch.py without a GPU: every case crosses its threshold at the smallest count, stays under what
the benchmark launches, its period keeps a 2^31 / 2^32-byte wrap off rows of equal content, and the comparison helper reports exactly
the element that differs."""
import pytest
import torch

from relax_vqa_amd.engine import VIT_CONFIGS
from tests import large_batch_cases as lb


@pytest.fixture(scope="module")
def vit(tmp_path_factory):
    """ViT-B/16's per-image sizes from the host library's geometry and arena exports"""
    return lb.vit_layout(lb.host_library(tmp_path_factory.mktemp("host")), VIT_CONFIGS["vit_base"][0], 16)


@pytest.fixture(scope="module")
def table(vit):
    return lb.cases(vit)


def test_vit_sizes_come_from_the_layout_export(vit):
    assert vit["ntok"] == 197 and vit["dim"] == 768
    assert (vit["hidden"], vit["hidden_x6"], vit["qkv"]) == (2420736, 3631104, 1815552)
    assert (vit["hidden_row"], vit["qkv_row"]) == (12288, 9216)
    assert vit["arena_planes"] == 9070080          # 9.1 MB per image (tests/test_vit_geometry_cpu.py)


def test_resnet_sizes_restated_from_the_geometry():
    assert lb.RN_CONV1_FLOATS * 4 == lb.RN_LAYER1_FLOATS * 4 == 3211264
    assert 28 * 28 * 512 * 4 == 1605632            # layer2's block output: 2^32 only from 2675 images, above the ceiling - no case


def test_every_case_crosses_its_threshold_at_the_smallest_count(table):
    assert {e["case"] for e in table} >= {"gemm_a", "gemm_out", "conv1x1", "conv3x3", "bn_relu_maxpool", "gap", "attention", "attention_ex",
                                          "vit_features", "vit_intermediate_layers", "resnet50_clip_features", "clip_vectors"}
    for e in table:
        assert e["threshold"] in lb.WRAPS
        assert e["unit_bytes"] * e["count"] >= e["threshold"], e
        if e["primary"]:
            assert e["unit_bytes"] * (e["count"] - e["slack"]) < e["threshold"], f"not the smallest count that crosses: {e}"
            assert e["slack"] == 16 or e["case"] in ("attention", "clip_vectors"), e
    assert all(any(e["primary"] for e in table if e["case"] == c) for c in {e["case"] for e in table})
    assert lb.GEMM_ROWS >= -(-2 ** 32 // 12288) == 349526
    assert all(lb.GEMM_ROWS % t for t in lb.TILE_SIZES), "the last tile is ragged at every tile height"


def test_no_case_is_larger_than_the_benchmark_launches(table):
    assert lb.CEILINGS == {"model": 2048, "operator": 403456, "images": 2048}
    for e in table:
        measure = e["rows"] if e["level"] == "operator" else e["count"]
        assert measure <= lb.CEILINGS[e["level"]], e
        assert e["level"] != "operator" or e["case"] in ("gemm_a", "gemm_out", "attention"), e
    assert lb.CLIPS * 2 * lb.CLIP_PAIRS == 1792 and lb.RN_IMAGES % 2 == 0
    # the 785-token case has narrower rows than anything the benchmark launches; in bytes and images it stays below the headline's qkv
    ex = next(e for e in table if e["case"] == "attention_ex")
    assert ex["unit_bytes"] * ex["count"] < 2048 * 1815552


def test_a_wrap_never_lands_on_equal_content(table):
    for e in table:
        p = e["period"]
        assert p > 1 and all(p % d for d in range(2, p)), f"period {p} is not a prime"
        assert all(t % p for t in lb.TILE_SIZES) and all(2 ** k % p for k in range(1, 40))
        for wrap in lb.WRAPS:
            assert not lb.wrap_lands_on_equal_content(e["unit_bytes"], p, wrap), e
            if wrap % e["unit_bytes"] == 0:          # a wrap by whole units: (2^32 / unit bytes) mod period != 0
                assert (wrap // e["unit_bytes"]) % p != 0, e
        # the pixel rows inside an image repeat with the image: in rows the period is (rows per image) x period
        if e["unit"] == "image" and e["unit_bytes"] % (e["rows"] // e["count"]) == 0:
            rows_per_image = e["rows"] // e["count"]
            row_bytes = e["unit_bytes"] // rows_per_image
            for wrap in lb.WRAPS:
                assert wrap % row_bytes or (wrap // row_bytes) % (rows_per_image * p) != 0, e
    assert lb.wrap_lands_on_equal_content(4096, 4, 2 ** 32) and not lb.wrap_lands_on_equal_content(4096, 7, 2 ** 32)      # the helper can say yes
    # resnet50_clip_features(both, n): the pool rows start at image n = 671 = 11 x 61, a whole number of periods
    assert (lb.RN_IMAGES // 2) % lb.PERIOD_IMAGES == 0


def _periodic(small, n, period, first=0):
    return small[lb.idx(torch.arange(first, first + n), period)].clone()


@pytest.mark.parametrize("dtype", [torch.float32, torch.int32])
def test_rows_equal_periodic_reports_exactly_the_flipped_element(dtype):
    g = torch.Generator().manual_seed(5)
    period, n, cols = 13, 1000, (6, 7)
    small = torch.randn((period,) + cols, generator=g).to(dtype) if dtype.is_floating_point else torch.randint(-99, 99, (period,) + cols, generator=g, dtype=dtype)
    big = _periodic(small, n, period)
    slice_bytes = 37 * 42 * 4            # 37 rows a slice: 28 slices, the last one ragged
    assert lb.rows_equal_periodic(big, small, period, slice_bytes=slice_bytes) is None
    assert lb.rows_equal_periodic(big, small, period) is None
    for row, col in ((n - 1, 41), (500, 17), (0, 0), (36, 41), (37, 0)):          # the last row; a middle slice; slice edges
        bad = big.clone()
        flat = bad.view(n, -1)
        flat[row, col] = flat[row, col] + 1
        got = lb.rows_equal_periodic(bad, small, period, slice_bytes=slice_bytes)
        assert got == (row, col, flat[row, col].item(), small.view(period, -1)[row % period, col].item()), (row, col, got)
    two = big.clone()
    two.view(n, -1)[700, 3] += 1
    two.view(n, -1)[200, 9] += 1
    assert lb.rows_equal_periodic(two, small, period, slice_bytes=slice_bytes)[:2] == (200, 9), "not the FIRST difference"
    # bits, not values: -0.0 against 0.0 differs, a NaN equals itself
    if dtype.is_floating_point:
        z = small.clone()
        z.view(period, -1)[4, 2] = 0.0
        bz = _periodic(z, n, period)
        bz.view(n, -1)[4 + period, 2] = -0.0
        assert lb.rows_equal_periodic(bz, z, period)[:2] == (4 + period, 2)
        z.view(period, -1)[4, 2] = float("nan")
        assert lb.rows_equal_periodic(_periodic(z, n, period), z, period) is None
    # rows that start inside a period (the pool rows of a two-group batch)
    assert lb.rows_equal_periodic(_periodic(small, 50, period, first=9), small, period, first=9) is None
    assert lb.rows_equal_periodic(_periodic(small, 50, period, first=9), small, period) is not None
    with pytest.raises(ValueError):
        lb.rows_equal_periodic(big, small[:, :5], period)


def test_rows_close_periodic_is_assert_close_on_the_expansion():
    from tests.gpu_common import assert_close
    g = torch.Generator().manual_seed(6)
    period, n = 11, 300
    small = torch.randn(period, 40, generator=g)
    big = _periodic(small, n, period)
    noisy = big * (1 + 8e-6 * (torch.rand(n, 40, generator=g) - 0.5))
    worst, row, col = lb.rows_close_periodic(noisy, small, period, 1e-5, 1e-5, slice_bytes=4096)
    assert 0 < worst <= 1.0
    assert_close(noisy, big.numpy(), "the same bound through assert_close", rtol=1e-5, atol_frac=1e-5)
    # the same ratio assert_close computes
    want = big.double()
    bound = 1e-5 * want.abs() + 1e-5 * (float(want.abs().mean()) + 1e-30)
    ratio = (noisy.double() - want).abs() / bound
    assert worst == pytest.approx(float(ratio.max()), rel=1e-9) and (row, col) == divmod(int(ratio.reshape(-1).argmax()), 40)
    noisy[n - 1, 39] *= 1.001
    worst, row, col = lb.rows_close_periodic(noisy, small, period, 1e-5, 1e-5, slice_bytes=4096)
    assert worst > 1.0 and (row, col) == (n - 1, 39)
    noisy[5, 5] = float("nan")
    assert lb.rows_close_periodic(noisy, small, period, 1e-5, 1e-5)[0] == float("inf")
