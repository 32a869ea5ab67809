"""``build_collector``: the collector ``Learner.configure(config, collector=...)`` takes, over the configuration's own
environments on the device."""


def build_collector(config):
    from prism_amd.collectors import VectorCollector
    from prism_amd.factory.env_factory import build_environment
    return VectorCollector(build_environment(config, config.num_processes), config)
