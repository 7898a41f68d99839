"""train.py --scene_images: parsing, the video key -> grid index mapping, and the errors for missing keys and bad shapes (CPU only)."""
import os

import numpy as np
import pytest

from desire_amd import train as T


class _Loader:
    """The two things scene_image_keys reads from a DataLoader."""
    def __init__(self, data_dir, leave):
        self.data_dir, self.leave_dataset = data_dir, leave

    def _csv_paths(self):
        from desire_amd.data_loader import DataLoader
        return DataLoader._csv_paths(self)


def _tree(tmp_path, videos):
    for v in videos:
        d = tmp_path / v
        d.mkdir(parents=True)
        (d / "annotations_processed.csv").write_text("")
    return str(tmp_path)


def test_parser_takes_scene_images():
    a = T.build_parser().parse_args(["--scene_images", "imgs.npz"])
    assert a.scene_images == "imgs.npz"
    assert T.build_parser().parse_args([]).scene_images is None


def test_video_keys_map_to_grid_indices(tmp_path):
    root = _tree(tmp_path, ["bookstore/video6", "bookstore/video0", "deathCircle/video4"])
    keys = T.scene_image_keys(_Loader(root, 3), root)
    assert keys == ["bookstore/video0", "bookstore/video6", "deathCircle/video4"]       # the loader's video order d
    G = 4
    imgs = {k: np.full((16, 16, 3), i, np.float32) for i, k in enumerate(["deathCircle/video4", "bookstore/video6", "bookstore/video0", "extra/v"])}
    path = str(tmp_path / "imgs.npz")
    np.savez(path, **imgs)
    images, gov = T.load_scene_images(path, keys, G, G)
    assert images.shape == (4, 16, 16, 3)                                               # n_grids = the file's entries, sorted by key
    order = sorted(imgs)
    assert [order[g] for g in gov] == keys
    for v, g in enumerate(gov):
        assert np.array_equal(images[g], imgs[keys[v]])
    assert list(T._gos(gov, [2, 0, 0, 1])) == [gov[2], gov[0], gov[0], gov[1]]
    assert T._gos(None, [0, 1]) is None


def test_missing_keys_and_bad_shapes_are_named(tmp_path):
    path = str(tmp_path / "imgs.npz")
    np.savez(path, **{"bookstore/video6": np.zeros((16, 16, 3), np.float32)})
    with pytest.raises(ValueError, match="deathCircle/video4"):
        T.load_scene_images(path, ["bookstore/video6", "deathCircle/video4"], 4, 4)
    np.savez(path, **{"bookstore/video6": np.zeros((16, 12, 3), np.float32), "a/b": np.zeros((16, 16, 3), np.float32)})
    with pytest.raises(ValueError, match=r"bookstore/video6 \(16, 12, 3\)"):
        T.load_scene_images(path, ["bookstore/video6"], 4, 4)
