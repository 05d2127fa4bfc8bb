"""Test-set loader on the device: CaptionUniPipeline.iter_test_batches over a TSV of JPEGs -- spawned decode workers, page-locked
shared-memory slabs (the only test in which hipHostRegister runs on them), the device transform -- gives, bit for bit, ImagePreprocessor
applied to decode_image of the same rows, and leaves no slab segment behind."""
import base64
import io
from multiprocessing import shared_memory

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [(48, 64), (33, 50), (64, 48), (50, 33), (40, 40)]


def _jpeg(h, w, seed):
    from PIL import Image
    g = np.random.default_rng(seed)
    base = g.integers(0, 256, size=(h // 8 + 2, w // 8 + 2, 3), dtype=np.uint8)
    buf = io.BytesIO()
    Image.fromarray(base, 'RGB').resize((w, h), Image.BILINEAR).save(buf, format='JPEG', quality=90)
    return base64.b64encode(buf.getvalue())


@pytest.mark.parametrize('device_jpeg', [True, False], ids=['device_jpeg', 'pillow_in_workers'])
def test_iter_test_batches_equals_preprocessed_decode(tmp_path, monkeypatch, device_jpeg):
    from vitcap_amd.imageio import ImagePreprocessor, decode_image
    from vitcap_amd.pipeline import CaptionUniPipeline
    from vitcap_amd.tsv import tsv_writer
    rows = [('img%d' % i, _jpeg(h, w, 40 + i)) for i, (h, w) in enumerate(SIZES)]
    tsv_writer(rows, str(tmp_path / 'test.tsv'))
    made = []

    class Recorded(shared_memory.SharedMemory):
        def __init__(self, name=None, create=False, size=0):
            super().__init__(name=name, create=create, size=size)
            if create:
                made.append(self.name)
    monkeypatch.setattr(shared_memory, 'SharedMemory', Recorded)
    pipe = CaptionUniPipeline(test_image_tsv=str(tmp_path / 'test.tsv'), test_batch_size=2, num_workers=2, device_jpeg=device_jpeg,
                              loader_slab_mb=1, test_crop_size=384, crop_pct=1.0)
    dev = torch.device('cuda', pipe.local_rank)
    pre = ImagePreprocessor(dev, 384, 1.0)
    keys = []
    for n, b in enumerate(pipe.iter_test_batches()):
        keys.append(b['key'])
        want = pre([decode_image(r[1]) for r in rows[2 * n:2 * n + 2]])
        image = b['image']
        assert image.dtype == torch.bfloat16 and image.shape == want.shape and image.device == want.device
        assert torch.equal(image, want), 'batch %d differs from the preprocessed decode' % n
    assert keys == [['img0', 'img1'], ['img2', 'img3'], ['img4']]
    assert len(made) == 15              # decode_ahead_plan(2, 2, 8, ...) = (1, 12, 15)
    for name in made:
        with pytest.raises(FileNotFoundError):
            shared_memory.SharedMemory(name=name)
