"""Images whose borders stress the border follower, shared by the GPU parity tests and the CPU tests of the follower tiers."""
import numpy as np


def sawtooth_frame(w, h, tooth, shapes):
    """White frame with dark rectangles whose edges are sawtoothed: borders with thousands of CHAIN_APPROX_SIMPLE points."""
    img = np.full((h, w), 220, np.uint8)
    for (x0, y0, x1, y1) in shapes:
        img[y0:y1, x0:x1] = 20
        for x in range(x0, x1, 2 * tooth):          # teeth along the top and bottom edges
            img[y0 - tooth:y0, x:x + tooth] = 20
            img[y1:y1 + tooth, x + tooth:x + 2 * tooth] = 20
        for y in range(y0, y1, 2 * tooth):          # and along the left and right edges
            img[y:y + tooth, x0 - tooth:x0] = 20
            img[y + tooth:y + 2 * tooth, x1:x1 + tooth] = 20
    return np.repeat(img[:, :, None], 3, axis=2)
