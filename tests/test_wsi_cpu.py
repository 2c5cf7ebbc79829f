"""§8f N4 oracle (oracle/ingest_oracle.region_tiles): the dzsave 'google' tile grid restated on the CPU."""
import numpy as np
import torch

from oracle.ingest_oracle import ingest, region_tiles


def test_region_tiles_are_padded_grid_crops():
    rng = np.random.default_rng(3)
    r = rng.integers(0, 256, size=(70, 100, 3), dtype=np.uint8)
    t, (ty, tx) = region_tiles(r, 32, 32)
    assert (ty, tx) == (3, 4) and t.shape == (12, 3, 32, 32)
    # interior tile: the crop itself / 255
    np.testing.assert_array_equal(t[5].numpy(), r[32:64, 32:64].transpose(2, 0, 1).astype(np.float32) / np.float32(255))
    # bottom-right tile: 6 valid rows, 4 valid columns, the rest background white
    last = t[11].numpy()
    np.testing.assert_array_equal(last[:, :6, :4], r[64:70, 96:100].transpose(2, 0, 1).astype(np.float32) / np.float32(255))
    assert (last[:, 6:, :] == 1.0).all() and (last[:, :, 4:] == 1.0).all()
    # the resize to the network size is the N1 chain on the padded tile
    t2, _ = region_tiles(r, 32, 24)
    pad = np.full((32, 32, 3), 255, np.uint8)
    pad[:6, :4] = r[64:70, 96:100]
    assert torch.equal(t2[11], ingest(pad, 24))


def test_region_tiles_halving_rounds_half_up():
    r = np.zeros((5, 6, 3), np.uint8)            # odd height: the last row is dropped (floor), as a 0.5 resize does
    r[0, 0], r[0, 1], r[1, 0], r[1, 1] = 1, 2, 2, 1   # mean 1.5 -> 2
    r[2:4, 2:4] = 255
    t, (ty, tx) = region_tiles(r, 4, 4, shrink=2)
    assert (ty, tx) == (1, 1)
    img = (t[0] * 255).round().numpy().astype(int)
    assert img[0, 0, 0] == 2 and img[0, 1, 1] == 255 and img[0, 0, 2] == 0
    assert (img[:, 2:, :] == 255).all() and (img[:, :, 3:] == 255).all()   # beyond the 2x3 halved image: background


# every public top-level name and upper-case constant of the single-file wsi module, before it became a package
WSI_SURFACE = """tile_grid wanted_tiles check_tile_mask probe_view StripStream RegionTileStream tissue_counts tissue_mask detect_region
evaluate_region BURDEN_MAX_CLASSES BURDEN_MAX_FIELDS BURDEN_MAX_FIELD_SIDE BURDEN_FLAG_NONFINITE BURDEN_FLAG_CLASS burden_map densest_fields
quantify_region PAIR_MAX_CLASSES PAIR_MAX_RADII PAIR_MAX_RADIUS_Q PAIR_MAX_SIDE spatial_radii_q spatial_roi_q pair_counts_device
spatial_summaries spatial_stats STAIN_BINS StainBasis H_DAB stain_tables StainStats StainMap stain_stats normalize_region BASIS_OD_SCALE
BASIS_OD_MAX BASIS_MOMENT_WORDS BASIS_DIR_BINS BASIS_STRIP basis_tables basis_plane basis_vectors StainEstimate estimate_basis LOAD_MIN_CELL
LOAD_MAX_SIDE LOAD_FLAG_NONFINITE LOAD_MAX_CELLS stain_load box_morphometry SEG_COLS SEG_MAX_SIDE SEG_MAX_MARGIN SEG_NONFINITE SEG_EMPTY
SEG_LARGE SEG_NOT_RESIDENT SEG_INTERNAL segment_boxes plaque_morphometry FOCUS_MIN_CELL FOCUS_MAX_SIDE FOCUS_FLAG_NONFINITE FOCUS_MAX_PIXELS
focus_map focus_summary SlideBatchPlan SlideSampler""".split()


def test_wsi_package_keeps_the_surface_and_holds_no_code():
    import inspect

    from amyloid_yolo_paper_amd import wsi
    assert len(WSI_SURFACE) == 69 and not [n for n in WSI_SURFACE if not hasattr(wsi, n)]
    # the package file re-exports: every function and class reachable as wsi.X is defined in a submodule (or outside the package)
    own = [n for n, v in vars(wsi).items() if (inspect.isfunction(v) or inspect.isclass(v)) and v.__module__ == wsi.__name__]
    assert own == []
