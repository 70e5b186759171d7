from .matcap import matcap_shader, matcap_sampler

__all__ = ["matcap_shader", "matcap_sampler"]
