"""Gene set files for ``cna.tl.gene_set_test``."""


def read_gmt(path):
    """The gene sets of a GMT file as a dict name -> list of gene names, in the file's order: one set per line, the
    name, a description (ignored), then the genes, separated by tabs.  Empty lines and empty gene fields are skipped; a
    line without a description field or a name that appears twice is a ValueError."""
    sets = {}
    with open(path) as f:
        for no, line in enumerate(f, 1):
            line = line.rstrip('\r\n')
            if not line.strip():
                continue
            fields = line.split('\t')
            name = fields[0].strip()
            if len(fields) < 2 or not name:
                raise ValueError('%s, line %d: a GMT line holds a name, a description and the genes, separated by tabs'
                                 % (path, no))
            if name in sets:
                raise ValueError('%s, line %d: the set %r appears twice' % (path, no, name))
            sets[name] = [g.strip() for g in fields[2:] if g.strip()]
    return sets
