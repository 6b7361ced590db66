"""hdrnet_amd -- MI355X-native BilateralSlice / BilateralSliceApply (google/hdrnet hot path).

Host side mirrors the reference's operator boundary:

* ``hdrnet_amd.hdrnet_ops``  <->  ``hdrnet/hdrnet_ops.py``  (bilateral_slice,
  bilateral_slice_apply and their registered gradients)
* ``hdrnet_amd.layers``      <->  the two slice wrappers of ``hdrnet/layers.py:99-148``
* ``hdrnet_amd.data``        <->  ``hdrnet/data_pipeline.py`` from the decoded image on (normalise, flip, rotate, crop,
  low-res copy), in one launch

Compute is hand-written HIP for gfx950 behind the C-ABI of ``include/hdrnet_amd.h``
(``hdrnet_amd/lib/libhdrnet_amd.so``).  PyTorch is used for device memory, streams
and ``torch.distributed`` only.
"""
from . import data, hdrnet_ops, layers  # noqa: F401
from .data import (DeviceDataset, RaggedDeviceDataset, draw_ops, lowres_input, pack_images, prepare_batch,  # noqa: F401
                   prepare_batch_ragged)
from .hdrnet_ops import bilateral_slice, bilateral_slice_apply  # noqa: F401

__version__ = "0.1.0"
