"""tests/fake_net.py's stand-in net, with the dtype of every frame it is given written down (model_path/dtypes.txt): the 16-bit
frame-pool test's proof that a "bit_depth": 16 task reaches the net as u16 samples."""
import os

import fake_net


class Net(fake_net.FakeNet):
    def submit_u8(self, img, out=None, tile_size=0, border=0):
        with open(os.path.join(os.path.dirname(self.journal), "dtypes.txt"), "a") as f:
            f.write("%d %s %s\n" % (int(img[0, 0, 0]), img.dtype, out.dtype))
        return super().submit_u8(img, out=out, tile_size=tile_size, border=border)


def make(model_path, model_file, scale, gpu):
    return Net(scale, journal=os.path.join(model_path, "journal.txt"))
