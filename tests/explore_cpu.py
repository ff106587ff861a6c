"""Plain-integer restatement of the exploration stream csrc/rgl_explore.hip carries per environment: numpy's legacy generator
seeded per case, advanced past the doubles scene generation took, then one `np.random.random()` per decision and, when it
explores, one `np.random.choice(n)` (numpy's masked rejection on 32-bit outputs).  Built on tests.scenegen_cpu.MT19937.

`ExploreStream(seed, draws).decide(greedy, n_actions, epsilon)` is one decision of a live environment; `words()` the 625 state
words the kernels keep (624 words and the position of the next one, 624 = twist first).  The counters say what a list of cases
met: twists in all, twists between the two words of random(), between random() and the choice, inside a rejection loop, and
rejected draws.
"""
import numpy as np

from tests.scenegen_cpu import MT19937

STATE_WORDS = 625


class ExploreStream(object):
    def __init__(self, seed, draws):
        self.rs = MT19937(int(seed))
        for _ in range(2 * max(int(draws), 0)):
            self.rs.next_u32()
        self.last_u = None
        self.twists = self.twist_inside_random = self.twist_before_choice = self.twist_in_rejection = self.rejections = 0

    def _next(self):
        """(output, whether taking it twisted the state first)"""
        twisted = self.rs.pos == 624
        self.twists += int(twisted)
        return self.rs.next_u32(), twisted

    def decide(self, greedy, n_actions, epsilon):
        a, _ = self._next()
        b, twisted = self._next()
        self.twist_inside_random += int(twisted)
        u = self.last_u = ((a >> 5) * 67108864 + (b >> 6)) / 9007199254740992.0
        if not u < epsilon:
            return int(greedy), 0
        if n_actions == 1:
            return 0, 1
        mask = n_actions - 1
        for shift in (1, 2, 4, 8, 16):
            mask |= mask >> shift
        first = True
        while True:
            w, twisted = self._next()
            if twisted and first:
                self.twist_before_choice += 1
            elif twisted:
                self.twist_in_rejection += 1
            first = False
            v = w & mask
            if v <= n_actions - 1:
                return v, 1
            self.rejections += 1

    def words(self):
        return np.array(self.rs.mt + [self.rs.pos], dtype=np.uint32)


def draws_for_position(pos, twists=1):
    """A draw count d after which ExploreStream(seed, d) stands at word `pos` (even, 0 meaning 624 words of the block spent: the
    state's position is then 624) of its `twists`-th block."""
    assert pos % 2 == 0 and 0 <= pos <= 624 and twists >= 1
    return (624 * (twists - 1) + (pos if pos else 624)) // 2
