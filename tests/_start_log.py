"""What the lazy resets of an overlay restatement (tests/_wind_oracle.py, _fruit_oracle.py, _doors_oracle.py, _boxes_oracle.py) drew:
how often each start cell, and how many times one step put two envs on different cells.  With one start cell -- or with too few
episodes ending -- a kernel's own copy of the start draw (the stream-1 prefix, the episode count) is compared on nothing: the tests on
grids with several starts assert on this log that it was."""
import numpy as np


class StartLog(object):
    def __init__(self, starts):
        self.cells = np.asarray(starts, np.int64)
        self.drawn = np.zeros(len(self.cells), np.int64)  # lazy resets per start cell, in the grid's order
        self.mixed = 0  # lazy-reset passes that put envs on more than one cell

    def note(self, pos):
        """pos: where one lazy-reset pass put the envs it reset."""
        hit = np.asarray(pos, np.int64)[:, None] == self.cells[None, :]
        assert hit.any(axis=1).all()  # a reset leads to a start cell
        per_cell = hit.sum(axis=0)
        self.drawn += per_cell
        self.mixed += int((per_cell > 0).sum() > 1)

    def every_start_was_drawn_and_some_step_mixed_them(self):
        return bool((self.drawn > 0).all() and self.mixed > 0)
