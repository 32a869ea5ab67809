"""``build_environment``: the environments of a configuration as ONE object of the ``VectorCollector`` protocol
(prism_amd/collectors.py).  Where the reference starts one process per environment
(its ``multiprocessing_experience_collection/environment_process.py:35-48``), MinAtar Breakout here is N
environments stepped by one launch on the learner's device (prism_amd/envs.py)."""

MINATAR_GAMES = ("Asterix", "Breakout", "Freeway", "Seaquest", "SpaceInvaders")


def build_environment(config, n_envs, seed=None):
    """``env_name`` "MinAtar/Breakout-v0" (six actions) or "MinAtar/Breakout-v1" (the minimal action set: no-op, left,
    right) -> ``DeviceBreakout``.  The other MinAtar games are not on the device: ``NotImplementedError`` naming the game.
    Anything else: ``ValueError``."""
    name = str(config.env_name)
    if "MinAtar/" not in name:
        raise ValueError(f"build_environment: no device environment for env_name = {name!r} (MinAtar/Breakout-v0 / -v1 only)")
    game = name.split("MinAtar/", 1)[1].split("-", 1)[0]
    if game != "Breakout":
        if game in MINATAR_GAMES:
            raise NotImplementedError(f"build_environment: MinAtar {game} is not implemented on the device (Breakout only)")
        raise ValueError(f"build_environment: unknown MinAtar game in env_name = {name!r}")
    from prism_amd.envs import DeviceBreakout
    return DeviceBreakout(n_envs, int(getattr(config, "seed", 0) if seed is None else seed), config.device,
                          sticky_action_prob=float(getattr(config, "atari_sticky_actions_prob", 0.0)),
                          episode_timestep_limit=int(getattr(config, "episode_timestep_limit", 0) or 0),
                          minimal_actions=name.endswith("-v1"))
