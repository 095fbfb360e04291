"""A scripted stand-in for griduniverse_amd.engine.Engine: the facade's host tests run against it without a device."""

ABSENT = dict(s=16, n_grids=1, overlay=0, overlay_bits=0, td_rows=0, double=0, dyna=0, sweep=0, explore=0, explore_c=0, mcts_nodes=0, mcts_c=0,
              ac=0, **{'is': 0}, fa_f=0, fa_k=0, trail_cap=0)
PRESENT = dict(ABSENT, td_rows=16, double=16, dyna=16, sweep=1, explore=16, explore_c=16, mcts_nodes=7, mcts_c=256, ac=16, **{'is': 16}, fa_f=16, fa_k=1)


class Scripted(object):
    """Stands in for Engine: records (method, positional arguments); stores() answers `held`."""

    def __init__(self, *a, **kw):
        self.calls, self.held = [], dict(ABSENT)

    def stores(self):
        self.calls.append(('stores', ()))
        return dict(self.held)

    def __getattr__(self, name):
        def call(*a, **kw):
            assert not kw, (name, kw)  # the facade passes everything by position
            self.calls.append((name, a))
            return {'read_trajectory': {}, 'read_stats': (None, None)}.get(name)
        return call
