"""The train-mode buffer layout (nefes_amd/csrc/layout.h nefes_train_off) for tests that drive the weight-gradient kernels with
plain buffers: a tile [rows x 128 samples] stores blocks of 32 rows x 16 samples contiguously,

    element (row, sample) at float offset [row / 32][sample / 16][row % 32][sample % 16].

to_device maps [tiles, rows, 128] in (row, sample) order to that order, from_device back.  tests/test_train_kernel_args.py holds
both against nefes_amd.train.rows_view and against the offset formula written out element by element."""


def train_off(row, sample):
    """layout.h nefes_train_off: float offset of (row, sample) inside a tile (ints or integer tensors)."""
    return ((row >> 5) * 8 + (sample >> 4)) * 512 + (row & 31) * 16 + (sample & 15)


def to_device(x):
    """[tiles, rows, 128] in (row, sample) order -> the same shape in device order (a copy); rows a multiple of 32."""
    T, rows, n = x.shape
    assert n == 128 and rows % 32 == 0, x.shape
    return x.reshape(T, rows // 32, 32, 8, 16).permute(0, 1, 3, 2, 4).reshape(T, rows, 128).contiguous()


def from_device(b):
    """the inverse of to_device (a copy)."""
    T, rows, n = b.shape
    assert n == 128 and rows % 32 == 0, b.shape
    return b.reshape(T, rows // 32, 8, 32, 16).permute(0, 1, 3, 2, 4).reshape(T, rows, 128).contiguous()
