"""Environment front-ends of the trainer (see vec_env.py for the VecEnv protocol)."""


def action_space_shape(space):
    """The action branches of an action space: one per ``nvec`` entry for a MultiDiscrete space, ``(n,)`` for any other
    (Discrete) space -- what the policy builds one head for each (upstream model.py:62)."""
    nvec = getattr(space, "nvec", None)
    if nvec is not None:
        shape = tuple(int(n) for n in nvec)
        if not shape or min(shape) <= 0:
            raise ValueError(f"MultiDiscrete action space with nvec {list(shape)}: every branch needs at least one action")
        return shape
    return (int(space.n),)
