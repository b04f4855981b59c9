"""What the tests of the batch mixing share (test_mix_rule.py, test_gpu_mix_batch.py): a case -- partner, lam, boxes, erase, erase values
-- once as the arguments of llcomp_amd.mix_samples and once as those of tests/mix_spec.py, and a batch between torch's [n, c, h, w] and
the bit patterns in either layout that the library takes."""
import mix_spec
from batch_support import NP_NAME, bits_of  # noqa: F401


def to_layout(t, layout):
    """torch [n, c, h, w] -> the bits as a numpy array in the layout, of the type mix_reference takes for the dtype"""
    b = mix_spec.bits(t if layout == "chw" else t.permute(0, 2, 3, 1))
    name = {v: k for k, v in mix_spec.DTYPES.items()}[t.dtype]
    return b.view(NP_NAME[name]) if name != "bfloat16" else b


class Case:
    """One call: what mix_spec.apply and mix_samples both take"""

    def __init__(self, partner=None, lam=None, boxes=None, erase=None, erase_value=None):
        self.partner, self.lam, self.boxes, self.erase, self.erase_value = partner, lam, boxes, erase, erase_value

    def samples(self, mi, n):
        return mi.mix_samples(n, partner=self.partner, lam=self.lam, boxes=self.boxes, erase=self.erase)

    def expected(self, batch, layout):
        """the spec's bits for the torch batch [n, c, h, w], in the layout"""
        out = mix_spec.apply(batch, self.partner, self.lam, self.boxes, self.erase, self.erase_value)
        return bits_of(to_layout(out, layout))

    def __repr__(self):
        return f"Case(partner={self.partner!r}, lam={self.lam!r}, boxes={self.boxes!r}, erase={self.erase!r}, erase_value={self.erase_value!r})"
