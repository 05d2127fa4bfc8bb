"""Host helpers for the attention maps of ImageCaptioning.attention_maps() / caption_with_maps(): the column layout of a map row
and views of its parts.  A row has width W = N_VIS + L (L = max_length): the visual keys in the engine's order, then the caption's
token keys, the probe's own key at column N_VIS + t, zeros behind it.  Works on torch tensors and numpy arrays alike."""

N_VIS = 578          # visual keys of an image
COL_TAG_CLS = 0      # tag_hidden[:, 0]
COL_ENC_CLS = 1      # the encoder's cls row
COL_PATCH0 = 2       # first of the 24 x 24 patches, row-major
GRID = 24
N_PATCH = GRID * GRID
COL_TEXT0 = N_VIS    # token key k at COL_TEXT0 + k (k < t), the probe itself at COL_TEXT0 + t
N_LAYERS = 4
N_HEADS = 12


def width(max_length):
    """Columns of a map row at this max_length."""
    return N_VIS + int(max_length)


def patch_grid(maps):
    """(..., W) -> the (..., 24, 24) view of the patch columns 2..577."""
    if maps.shape[-1] < N_VIS:
        raise ValueError('patch_grid: the last dimension (%d) holds no %d visual columns' % (maps.shape[-1], N_VIS))
    return maps[..., COL_PATCH0:COL_PATCH0 + N_PATCH].reshape(tuple(maps.shape[:-1]) + (GRID, GRID))


def text_mass(maps, L):
    """(..., W) -> (...): the probability on the text keys (token keys and the probe itself), the sum over columns 578.."""
    if maps.shape[-1] != width(L):
        raise ValueError('text_mass: the last dimension is %d, max_length %d has %d columns' % (maps.shape[-1], int(L), width(L)))
    return maps[..., COL_TEXT0:].sum(-1)
