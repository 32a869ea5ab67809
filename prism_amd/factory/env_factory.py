"""``build_environment``: the environments of a configuration as ONE object of the ``VectorCollector`` protocol
(prism_amd/collectors.py).  Where the reference starts one process per environment
(its ``multiprocessing_experience_collection/environment_process.py:35-48``), a MinAtar game here is N environments
stepped by one launch on the learner's device (prism_amd/envs.py)."""

MINATAR_GAMES = ("Asterix", "Breakout", "Freeway", "Seaquest", "SpaceInvaders")
DEVICE_GAMES = {"Breakout": "DeviceBreakout", "Freeway": "DeviceFreeway", "Asterix": "DeviceAsterix",
                "SpaceInvaders": "DeviceSpaceInvaders"}          # game -> its class in prism_amd/envs.py
DEFAULT_DEVICE_GAMES = ("Breakout",)
# the games whose state record is wider than the 8 words of DEVICE_GAMES: a registry and a knob of their own
WIDE_DEVICE_GAMES = {"Seaquest": "DeviceSeaquest"}
DEFAULT_WIDE_DEVICE_GAMES = ()


def enabled_games(config):
    """``config.device_env_games`` (a plain attribute, default ``("Breakout",)``): the games ``build_environment`` may put on
    the device.  A name that is no device game is a ``ValueError``."""
    games = getattr(config, "device_env_games", DEFAULT_DEVICE_GAMES)
    games = (games,) if isinstance(games, str) else tuple(games)
    for g in games:
        if g not in DEVICE_GAMES:
            raise ValueError(f"build_environment: device_env_games names {g!r}; the device games are {sorted(DEVICE_GAMES)}")
    return games


def enabled_wide_games(config):
    """``config.device_env_wide_games`` (a plain attribute, default ``()``): the wide-record games ``build_environment`` may
    put on the device.  A name that is no wide game is a ``ValueError``."""
    games = getattr(config, "device_env_wide_games", DEFAULT_WIDE_DEVICE_GAMES)
    games = (games,) if isinstance(games, str) else tuple(games)
    for g in games:
        if g not in WIDE_DEVICE_GAMES:
            raise ValueError(f"build_environment: device_env_wide_games names {g!r}; the wide-record device games are "
                             f"{sorted(WIDE_DEVICE_GAMES)}")
    return games


def build_environment(config, n_envs, seed=None):
    """``env_name`` "MinAtar/Breakout-v0" (six actions) or "MinAtar/Breakout-v1" (the minimal action set: no-op, left,
    right) -> ``DeviceBreakout``; with "Freeway" in ``config.device_env_games``, "MinAtar/Freeway-v0" / "-v1" (no-op, up,
    down) -> ``DeviceFreeway``; with "Asterix" in it, "MinAtar/Asterix-v0" / "-v1" (five actions: no-op, left, up, right,
    down) -> ``DeviceAsterix``; with "SpaceInvaders" in it, "MinAtar/SpaceInvaders-v0" / "-v1" (four actions: no-op, left,
    right, fire) -> ``DeviceSpaceInvaders``; with "Seaquest" in ``config.device_env_wide_games``, "MinAtar/Seaquest-v0" /
    "-v1" (six actions either way) -> ``DeviceSeaquest``.  A MinAtar game that is not on the device, or not enabled:
    ``NotImplementedError`` naming the game.  Anything else: ``ValueError``."""
    name = str(config.env_name)
    if "MinAtar/" not in name:
        raise ValueError(f"build_environment: no device environment for env_name = {name!r} (MinAtar/Breakout, MinAtar/Freeway, "
                         "MinAtar/Asterix and MinAtar/SpaceInvaders, -v0 / -v1, only)")
    game = name.split("MinAtar/", 1)[1].split("-", 1)[0]
    games, wide = enabled_games(config), enabled_wide_games(config)
    if game in wide:
        cls = WIDE_DEVICE_GAMES[game]
    elif game in games:
        cls = DEVICE_GAMES[game]
    else:
        if game in DEVICE_GAMES:
            raise NotImplementedError(f"build_environment: MinAtar {game} on the device is opt-in: add {game!r} to "
                                      f"config.device_env_games (default {DEFAULT_DEVICE_GAMES!r})")
        if game in MINATAR_GAMES:
            raise NotImplementedError(f"build_environment: MinAtar {game} is not implemented on the device "
                                      f"({' and '.join(sorted(DEVICE_GAMES))} only) unless config.device_env_wide_games names it "
                                      f"(the wide-record games: {sorted(WIDE_DEVICE_GAMES)}; default {DEFAULT_WIDE_DEVICE_GAMES!r})")
        raise ValueError(f"build_environment: unknown MinAtar game in env_name = {name!r}")
    from prism_amd import envs
    return getattr(envs, cls)(n_envs, int(getattr(config, "seed", 0) if seed is None else seed), config.device,
                              sticky_action_prob=float(getattr(config, "atari_sticky_actions_prob", 0.0)),
                              episode_timestep_limit=int(getattr(config, "episode_timestep_limit", 0) or 0),
                              minimal_actions=name.endswith("-v1"))
